// dq_ingest.cpp -- host-resident Arrow batches into HBM for dq_scan, without a JVM.
//
// Reference seam: AnalysisRunner.runScanningAnalyzers hands Spark's DataFrame to data.agg(...)
// (analyzers/runners/AnalysisRunner.scala:279-326); a drop-in shim receives the columns as Arrow record
// batches (Spark's ArrowColumnVector / toArrow export, pyarrow, arrow-rs all speak the Arrow C Data
// Interface).  dq_arrow_import maps one exported ArrowArray / ArrowSchema to the host buffers of a
// dq column; dq_upload moves a chunk of such columns into device memory through pinned staging
// buffers, double- (n-) buffered so the copy of chunk k + 1 overlaps the scan of chunk k:
//
//     host Arrow buffers --(CPU threads, memcpy)--> pinned slot s --(DMA, copy stream)--> device slot s
//     scan stream: waits for the slot's copy (dq_upload_fence), scans, then frees the slot (dq_upload_release)
//
// The CPU copy into pinned memory is what lets the DMA engine stream at full PCIe rate from pageable
// Arrow memory; a slot is reused only after the scan that read it has passed its release event.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <atomic>
#include <climits>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/dqscan.h"
#include "dq_internal.h"
#include "dq_upload_host.h"

using dq::set_error;

namespace {

using namespace dq::up;  // the copy pieces and their thread pool (dq_upload_host.h, shared with dq_upload_stage)

int32_t type_of_format(const char* f) {
  if (!f) return 0;
  if (std::strcmp(f, "g") == 0) return DQ_TYPE_F64;
  if (std::strcmp(f, "l") == 0) return DQ_TYPE_I64;
  if (std::strcmp(f, "i") == 0) return DQ_TYPE_I32;
  if (std::strcmp(f, "u") == 0) return DQ_TYPE_UTF8;
  if (std::strcmp(f, "U") == 0) return DQ_TYPE_LARGE_UTF8;
  if (std::strcmp(f, "f") == 0) return DQ_TYPE_F32;
  if (std::strcmp(f, "s") == 0) return DQ_TYPE_I16;
  if (std::strcmp(f, "c") == 0) return DQ_TYPE_I8;
  if (std::strcmp(f, "b") == 0) return DQ_TYPE_BOOL;
  if (std::strcmp(f, "tdD") == 0) return DQ_TYPE_DATE32;
  // timestamp[us, tz]: Spark's TimestampType is UTC microseconds whatever the session zone (other units are not
  // TimestampType values: a producer converts them)
  if (std::strncmp(f, "tsu:", 4) == 0) return DQ_TYPE_TIMESTAMP;
  // decimal128 "d:precision,scale[,128]" (Spark's DecimalType(p, s); no negative scales, no 256-bit width)
  if (f[0] == 'd' && f[1] == ':') {
    int p = -1, sc = -1, w = 128, n = 0;
    const int k = std::sscanf(f + 2, "%d,%d%n", &p, &sc, &n);
    if (k != 2) return 0;
    const char* rest = f + 2 + n;
    if (*rest == ',') {
      if (std::sscanf(rest + 1, "%d", &w) != 1) return 0;
    } else if (*rest != '\0') {
      return 0;
    }
    if (w != 128 || p < 1 || p > dq::kDecMaxPrecision || sc < 0 || sc > p) return 0;
    return DQ_DECIMAL128(p, sc);
  }
  return 0;
}

}  // namespace

struct dq_uploader {
  int device = 0;
  int threads = 8;
  int64_t slot_bytes = 0;
  std::vector<char*> pinned, dev;
  std::vector<hipEvent_t> copied, released;
  std::vector<bool> used;
  hipStream_t copy = nullptr;
  int64_t next = 0;  // chunks uploaded
  double host_ms = 0.0;
  int64_t bytes = 0;
};

extern "C" {

dq_status dq_arrow_import(const struct ArrowSchema* schema, const struct ArrowArray* array, dq_host_column* out) {
  if (!schema || !array || !out) return set_error(DQ_E_INVALID, "dq_arrow_import: bad argument");
  if (!schema->release || !array->release) return set_error(DQ_E_INVALID, "dq_arrow_import: released Arrow structure");
  const int32_t type = type_of_format(schema->format);
  if (!type)
    return set_error(DQ_E_UNSUPPORTED, "Arrow format '%s' is not a GPU column type (g, f, l, i, s, c, b, tdD, tsu:, d:p,s, u, U)",
                     schema->format ? schema->format : "(null)");
  if (schema->n_children != 0 || array->n_children != 0 || schema->dictionary || array->dictionary)
    return set_error(DQ_E_UNSUPPORTED, "nested / dictionary-encoded Arrow arrays are not GPU columns");
  const bool str = type == DQ_TYPE_UTF8 || type == DQ_TYPE_LARGE_UTF8;
  if (array->n_buffers != (str ? 3 : 2) || !array->buffers)
    return set_error(DQ_E_INVALID, "Arrow array of format '%s' with %lld buffers", schema->format,
                     (long long)array->n_buffers);
  const int64_t n = array->length, off = array->offset;
  if (n < 0 || off < 0) return set_error(DQ_E_INVALID, "Arrow array with negative length / offset");
  dq_host_column c{};
  c.type = type;
  c.n_rows = n;
  if (n == 0) {  // producers may export NULL buffers for an empty array: touch none
    *out = c;
    return DQ_OK;
  }
  const uint8_t* validity = static_cast<const uint8_t*>(array->buffers[0]);
  if (array->null_count == 0) validity = nullptr;  // buffers[0] may be NULL then
  if (array->null_count != 0 && !validity && array->null_count != -1)
    return set_error(DQ_E_INVALID, "Arrow array with %lld nulls and no validity buffer", (long long)array->null_count);
  if (!array->buffers[1]) return set_error(DQ_E_INVALID, "Arrow array of format '%s' without its %s buffer",
                                           schema->format, str ? "offsets" : "values");
  c.nullable = validity ? 1 : 0;
  // a slice (RecordBatch.slice, to_batches(max_chunksize)): row 0 is bit off % 8 of byte off / 8; dq_upload
  // shifts the bitmap into place while it copies (a boolean array's value bits too)
  const bool bits = type == DQ_TYPE_BOOL;
  c.validity = validity ? validity + off / 8 : nullptr;
  c.validity_bytes = validity ? (n + 7) / 8 : 0;
  c.validity_bit = validity || bits ? (int32_t)(off & 7) : 0;
  if (bits) {
    c.values = static_cast<const char*>(array->buffers[1]) + off / 8;
    c.value_bytes = (n + 7) / 8;
    c.offsets = nullptr;
    c.offset_bytes = 0;
  } else if (!str) {
    const int64_t w = value_width(type);
    c.values = static_cast<const char*>(array->buffers[1]) + off * w;
    c.value_bytes = n * w;
    c.offsets = nullptr;
    c.offset_bytes = 0;
  } else {
    const int64_t w = type == DQ_TYPE_UTF8 ? 4 : 8;
    const char* offs = static_cast<const char*>(array->buffers[1]) + off * w;
    int64_t o0, o1;
    if (w == 4) {
      o0 = reinterpret_cast<const int32_t*>(offs)[0];
      o1 = reinterpret_cast<const int32_t*>(offs)[n];
    } else {
      o0 = reinterpret_cast<const int64_t*>(offs)[0];
      o1 = reinterpret_cast<const int64_t*>(offs)[n];
    }
    if (o0 < 0 || o1 < o0) return set_error(DQ_E_INVALID, "Arrow string offsets %lld..%lld", (long long)o0, (long long)o1);
    if (o1 > o0 && !array->buffers[2]) return set_error(DQ_E_INVALID, "Arrow string array without its data buffer");
    // a slice's offsets start at o0: dq_upload copies the bytes from o0 and writes offsets - o0
    c.offsets = offs;
    c.offset_bytes = (n + 1) * w;
    c.offset_base = o0;
    c.values = o1 > o0 ? static_cast<const char*>(array->buffers[2]) + o0 : nullptr;
    c.value_bytes = o1 - o0;
  }
  *out = c;
  return DQ_OK;
}

dq_status dq_arrow_import_dictionary(const struct ArrowSchema* schema, const struct ArrowArray* array,
                                     dq_host_column* indices, dq_host_column* dictionary) {
  const char* me = "dq_arrow_import_dictionary";
  if (!schema || !array || !indices || !dictionary) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (!schema->release || !array->release) return set_error(DQ_E_INVALID, "%s: released Arrow structure", me);
  if (!schema->dictionary || !array->dictionary) return set_error(DQ_E_INVALID, "%s: not a dictionary-encoded array", me);
  if (schema->n_children != 0 || array->n_children != 0) return set_error(DQ_E_UNSUPPORTED, "%s: nested Arrow array", me);
  const char* f = schema->format ? schema->format : "";
  int32_t itype = 0, is_unsigned = 0;
  if (std::strcmp(f, "c") == 0) itype = DQ_TYPE_I8;
  else if (std::strcmp(f, "s") == 0) itype = DQ_TYPE_I16;
  else if (std::strcmp(f, "i") == 0) itype = DQ_TYPE_I32;
  else if (std::strcmp(f, "C") == 0) itype = DQ_TYPE_I8, is_unsigned = 1;
  else if (std::strcmp(f, "S") == 0) itype = DQ_TYPE_I16, is_unsigned = 1;
  else return set_error(DQ_E_UNSUPPORTED, "%s: dictionary indices of Arrow format '%s' (c, s, i, C, S)", me, f);
  const char* df = schema->dictionary->format ? schema->dictionary->format : "";
  if (std::strcmp(df, "u") != 0 && std::strcmp(df, "U") != 0)
    return set_error(DQ_E_UNSUPPORTED, "%s: dictionary values of Arrow format '%s' (u, U)", me, df);
  // the values: an ordinary string array (dq_arrow_import refuses a nested dictionary and honours a slice)
  dq_host_column d{};
  if (dq_status s = dq_arrow_import(schema->dictionary, array->dictionary, &d)) return s;
  // the indices: the fixed-width array the format names, without the dictionary members
  struct ArrowSchema is = *schema;
  struct ArrowArray ia = *array;
  is.dictionary = nullptr;
  ia.dictionary = nullptr;
  is.format = itype == DQ_TYPE_I8 ? "c" : itype == DQ_TYPE_I16 ? "s" : "i";
  dq_host_column x{};
  if (dq_status s = dq_arrow_import(&is, &ia, &x)) return s;
  // the index column as dq_upload takes it: DQ_TYPE_DICT_UTF8, 4 bytes per row on the device, the source width
  // in `reserved` (dq_dict_check_indices' type code: negative = unsigned), the entry count in `offset_base`
  x.reserved = is_unsigned ? -itype : itype;
  x.type = DQ_TYPE_DICT_UTF8;
  x.value_bytes = 4 * x.n_rows;
  x.offset_base = d.n_rows;
  *indices = x;
  *dictionary = d;
  return DQ_OK;
}

dq_status dq_dict_check_indices(int32_t index_type, const void* indices, int64_t n, const uint8_t* validity,
                                int32_t validity_bit, int64_t n_entries, int32_t* out) {
  if (n < 0 || n_entries < 0 || validity_bit < 0 || validity_bit > 7 || (n > 0 && !indices))
    return set_error(DQ_E_INVALID, "dq_dict_check_indices: bad argument");
  if (!index_type_ok(index_type)) return set_error(DQ_E_UNSUPPORTED, "dq_dict_check_indices: index type %d", index_type);
  int64_t v = 0;
  const int64_t r = widen_check(index_type, indices, 0, n, validity, validity_bit, n_entries, out, &v);
  if (r >= 0)
    return set_error(DQ_E_INVALID, "dictionary index %lld at row %lld is outside the dictionary's %lld entries",
                     (long long)v, (long long)r, (long long)n_entries);
  return DQ_OK;
}

dq_status dq_uploader_create(int32_t device, int32_t n_slots, int64_t slot_bytes, int32_t host_threads,
                             dq_uploader** out) {
  if (!out || n_slots < 1 || n_slots > 8 || slot_bytes <= 0) return set_error(DQ_E_INVALID, "dq_uploader_create: bad argument");
  dq_uploader* u = new dq_uploader();
  u->device = device;
  u->threads = host_threads > 0 ? host_threads : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  u->slot_bytes = align_up(slot_bytes);
  auto fail = [&](hipError_t e, const char* what) {
    dq_uploader_destroy(u);
    return set_error(e == hipErrorOutOfMemory ? DQ_E_OOM : DQ_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(e, "hipSetDevice");
  if ((e = hipStreamCreateWithFlags(&u->copy, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  for (int s = 0; s < n_slots; ++s) {
    char* h = nullptr;
    char* d = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&h), (size_t)u->slot_bytes, hipHostMallocDefault)) != hipSuccess)
      return fail(e, "hipHostMalloc");
    u->pinned.push_back(h);
    if ((e = hipMalloc(reinterpret_cast<void**>(&d), (size_t)u->slot_bytes)) != hipSuccess) return fail(e, "hipMalloc");
    u->dev.push_back(d);
    if ((e = hipEventCreateWithFlags(&a, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
    u->copied.push_back(a);
    if ((e = hipEventCreateWithFlags(&b, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
    u->released.push_back(b);
    u->used.push_back(false);
  }
  *out = u;
  return DQ_OK;
}

dq_status dq_upload(dq_uploader* u, const dq_host_column* cols, int32_t n_cols, dq_column_view* dev_views) {
  if (!u || (n_cols > 0 && (!cols || !dev_views)) || n_cols < 0) return set_error(DQ_E_INVALID, "dq_upload: bad argument");
  const int s = (int)(u->next % (int64_t)u->pinned.size());
  // layout of the slot
  std::vector<Piece> pieces;
  int64_t at = 0;
  std::vector<int64_t> pos(3 * (size_t)n_cols, -1);
  for (int32_t c = 0; c < n_cols; ++c) {
    const dq_host_column& h = cols[c];
    if (h.validity_bit < 0 || h.validity_bit > 7 || h.offset_base < 0)
      return set_error(DQ_E_INVALID, "dq_upload: column %d: bad slice rebase", c);
    if (h.type == DQ_TYPE_DICT_UTF8 && (!index_type_ok(h.reserved) || h.offsets || h.value_bytes != 4 * h.n_rows))
      return set_error(DQ_E_INVALID, "dq_upload: column %d: not a dictionary index column of dq_arrow_import_dictionary", c);
    const void* src[3] = {h.values, h.validity, h.offsets};
    const int64_t len[3] = {h.value_bytes, h.validity_bytes, h.offset_bytes};
    for (int k = 0; k < 3; ++k) {
      if (!src[k] || len[k] <= 0) continue;
      pos[3 * (size_t)c + k] = at;
      at = align_up(at + len[k]);
    }
  }
  if (at > u->slot_bytes)
    return set_error(DQ_E_INVALID, "dq_upload: chunk needs %lld bytes, slot holds %lld", (long long)at,
                     (long long)u->slot_bytes);
  hipError_t e = hipSetDevice(u->device);
  if (e != hipSuccess) return set_error(DQ_E_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
  // the slot's previous DMA must have drained the pinned buffer before the CPU overwrites it
  if (u->used[(size_t)s] && (e = hipEventSynchronize(u->copied[(size_t)s])) != hipSuccess)
    return set_error(DQ_E_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(e));
  std::vector<std::atomic<int64_t>> bad((size_t)std::max(1, n_cols));
  for (auto& b : bad) b.store(INT64_MAX);
  for (int32_t c = 0; c < n_cols; ++c) {
    const dq_host_column& h = cols[c];
    const void* src[3] = {h.values, h.validity, h.offsets};
    const int64_t len[3] = {h.value_bytes, h.validity_bytes, h.offset_bytes};
    for (int k = 0; k < 3; ++k) {
      if (pos[3 * (size_t)c + k] < 0) continue;
      Piece p{u->pinned[(size_t)s] + pos[3 * (size_t)c + k], static_cast<const char*>(src[k]), len[k]};
      if (k == 0 && h.type == DQ_TYPE_DICT_UTF8) {  // narrow indices -> int32, validated in the same loop
        p.kind = 4;
        p.idx_type = h.reserved;
        p.n_entries = h.offset_base;
        p.valid = h.validity;
        p.valid_bit = h.validity_bit;
        p.bad = &bad[(size_t)c];
      }
      if ((k == 1 || (k == 0 && h.type == DQ_TYPE_BOOL)) && h.validity_bit) {  // bitmaps of a slice
        p.kind = 3;
        p.shift = h.validity_bit;
        p.src_bytes = (h.validity_bit + h.n_rows + 7) / 8;
      }
      if (k == 2 && h.offset_base) {
        p.kind = h.type == DQ_TYPE_UTF8 ? 1 : 2;
        p.base = h.offset_base;
      }
      pieces.push_back(p);
    }
  }
  parallel_copy(pieces, u->threads);
  for (int32_t c = 0; c < n_cols; ++c) {  // an index outside its dictionary: nothing is uploaded or scanned
    const int64_t r = bad[(size_t)c].load();
    if (r == INT64_MAX) continue;
    int64_t v = 0;
    (void)widen_check(cols[c].reserved, cols[c].values, r, r + 1, cols[c].validity, cols[c].validity_bit,
                      cols[c].offset_base, nullptr, &v);
    return set_error(DQ_E_INVALID, "dq_upload: column %d: dictionary index %lld at row %lld is outside the dictionary's "
                     "%lld entries", c, (long long)v, (long long)r, (long long)cols[c].offset_base);
  }
  // the scan that last read the device slot must have passed its release before the DMA overwrites it
  if (u->used[(size_t)s] && (e = hipStreamWaitEvent(u->copy, u->released[(size_t)s], 0)) != hipSuccess)
    return set_error(DQ_E_HIP, "hipStreamWaitEvent failed: %s", hipGetErrorString(e));
  if (at > 0 && (e = hipMemcpyAsync(u->dev[(size_t)s], u->pinned[(size_t)s], (size_t)at, hipMemcpyHostToDevice, u->copy)) !=
                    hipSuccess)
    return set_error(DQ_E_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
  if ((e = hipEventRecord(u->copied[(size_t)s], u->copy)) != hipSuccess)
    return set_error(DQ_E_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  for (int32_t c = 0; c < n_cols; ++c) {
    char* base = u->dev[(size_t)s];
    const int64_t* p = &pos[3 * (size_t)c];
    dev_views[c].values = p[0] >= 0 ? base + p[0] : nullptr;
    dev_views[c].validity = p[1] >= 0 ? reinterpret_cast<const uint8_t*>(base + p[1]) : nullptr;
    dev_views[c].offsets = p[2] >= 0 ? base + p[2] : nullptr;
    dev_views[c].reserved = 0;
  }
  u->used[(size_t)s] = true;
  u->bytes += at;
  ++u->next;
  return DQ_OK;
}

dq_status dq_upload_to(dq_uploader* u, const dq_host_column* cols, int32_t n_cols, const dq_upload_dest* dests) {
  if (!u || (n_cols > 0 && (!cols || !dests)) || n_cols < 0) return set_error(DQ_E_INVALID, "dq_upload_to: bad argument");
  const size_t s = (size_t)(u->next % (int64_t)u->pinned.size());
  hipError_t e = hipSetDevice(u->device);
  if (e != hipSuccess) return set_error(DQ_E_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
  // the slot's previous DMA must have drained the pinned buffer before the CPU overwrites it
  if (u->used[s] && (e = hipEventSynchronize(u->copied[s])) != hipSuccess)
    return set_error(DQ_E_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(e));
  std::vector<int64_t> pos(3 * (size_t)std::max(1, n_cols), -1);
  int64_t at = 0;
  if (dq_status st = stage(cols, n_cols, dests, u->pinned[s], u->slot_bytes, u->threads, pos.data(), &at))
    return st;
  // one DMA per destination buffer, its whole image (rows and padding); the device slot is not used
  for (int32_t c = 0; c < n_cols; ++c) {
    void* dst[3] = {dests[c].values, dests[c].validity, dests[c].offsets};
    const int64_t len[3] = {dests[c].value_bytes, dests[c].validity_bytes, dests[c].offset_bytes};
    for (int k = 0; k < 3; ++k) {
      const int64_t p = pos[3 * (size_t)c + k];
      if (p < 0) continue;
      if ((e = hipMemcpyAsync(dst[k], u->pinned[s] + p, (size_t)len[k], hipMemcpyHostToDevice, u->copy)) != hipSuccess)
        return set_error(DQ_E_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
    }
  }
  if ((e = hipEventRecord(u->copied[s], u->copy)) != hipSuccess)
    return set_error(DQ_E_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  u->used[s] = true;
  u->bytes += at;
  ++u->next;
  return DQ_OK;
}

dq_status dq_upload_fence(dq_uploader* u, void* hip_stream) {
  if (!u || u->next == 0) return set_error(DQ_E_INVALID, "dq_upload_fence: nothing uploaded");
  const size_t s = (size_t)((u->next - 1) % (int64_t)u->pinned.size());
  const hipError_t e = hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), u->copied[s], 0);
  return e == hipSuccess ? DQ_OK : set_error(DQ_E_HIP, "hipStreamWaitEvent failed: %s", hipGetErrorString(e));
}

dq_status dq_upload_release(dq_uploader* u, void* hip_stream) {
  if (!u || u->next == 0) return set_error(DQ_E_INVALID, "dq_upload_release: nothing uploaded");
  const size_t s = (size_t)((u->next - 1) % (int64_t)u->pinned.size());
  const hipError_t e = hipEventRecord(u->released[s], static_cast<hipStream_t>(hip_stream));
  return e == hipSuccess ? DQ_OK : set_error(DQ_E_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
}

dq_status dq_upload_sync(dq_uploader* u) {
  if (!u) return set_error(DQ_E_INVALID, "dq_upload_sync: bad argument");
  const hipError_t e = hipStreamSynchronize(u->copy);
  return e == hipSuccess ? DQ_OK : set_error(DQ_E_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
}

void dq_uploader_destroy(dq_uploader* u) {
  if (!u) return;
  (void)hipSetDevice(u->device);
  if (u->copy) (void)hipStreamSynchronize(u->copy);
  for (char* h : u->pinned) (void)hipHostFree(h);
  for (char* d : u->dev) (void)hipFree(d);
  for (hipEvent_t e : u->copied) (void)hipEventDestroy(e);
  for (hipEvent_t e : u->released) (void)hipEventDestroy(e);
  if (u->copy) (void)hipStreamDestroy(u->copy);
  delete u;
}

}  // extern "C"
