// dq_plan_host.h -- what the host translation units of the fused scan share (dq_plan.cpp, dq_rowprog.cpp,
// dq_pred_lower.cpp): the kernels' launchers, the column type predicates, and the one copy of what the predicate
// pass and the row-outcome pass must size and fill alike.  Host only: no .hip file includes it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "dq_device.h"
#include "dq_hip_host.h"

// rows per range at least this many: below it a launch's time goes to dispatching workgroups and to their
// fixed work (shift search, reductions, partial records), not to the rows -- a 10 M-row chunk (C1) otherwise
// ran 4-12 K workgroups of 2-4 K rows; every chunk of >= 16 K x 8192 rows is unaffected
#ifndef DQ_MIN_RANGE_ROWS
#define DQ_MIN_RANGE_ROWS 16384
#endif
// predicate-pass workgroups per chunk (A/B builds: -DDQ_PRED_WGS=...)
#ifndef DQ_PRED_WGS
#define DQ_PRED_WGS 2048
#endif

namespace dq {

hipError_t launch_pred_scan(const PredProgram* prog, const ScanCols& cols, const ScanBitmaps& bm, int64_t n_rows,
                            int64_t rows_per_range, int32_t nranges, PredPartial* acc, int32_t lds_bytes, hipStream_t st,
                            bool has_regex);
hipError_t launch_row_outcomes(const PredProgram* prog, const ScanCols& cols, uint32_t* const* pass,
                               uint32_t* const* applies, int32_t n_out, int64_t n_rows, int64_t rows_per_range,
                               int32_t nranges, PredPartial* acc, int32_t lds_bytes, hipStream_t st, bool has_regex);
hipError_t launch_column_scan(int32_t variant, const ColTask* tasks, int32_t ntasks, int32_t part_base,
                              const ScanCols& cols, const ScanBitmaps& bm, int64_t n_rows, int64_t rows_per_range,
                              int32_t nranges, ColPartial* partials, uint32_t* hll_acc, const uint32_t* hll_floor,
                              bool long_str, hipStream_t st);
hipError_t launch_pair_scan(const PairWG* wgs, int32_t nwg, const ScanCols& cols, const ScanBitmaps& bm,
                            const uint32_t* ones, int64_t n_rows, int64_t rows_per_range, int32_t nranges,
                            CorrPartial* pair_part, ColPartial* col_part, int32_t* redo, bool all_f64, bool ring,
                            bool minmax, hipStream_t st);
hipError_t pair_scan_residency(bool all_f64, bool ring, bool minmax, int32_t* per_cu);
hipError_t launch_finalize(int32_t ncol, int32_t nranges_col, const ColPartial* col_part, ColPartial* col_acc,
                           int32_t npair, int32_t nranges_pair, const CorrPartial* pair_part, CorrPartial* pair_acc,
                           int32_t has_pred, int32_t nranges_pred, const PredPartial* pred_part, PredPartial* pred_acc, const FinRanges& fr, int64_t* rare_dev, int64_t* rare_host,
                           int32_t nhll, const uint32_t* hll_acc, uint32_t* hll_floor, hipStream_t st);
hipError_t launch_dict_scan(const ColTask* tasks, int32_t ntasks, int32_t part_base, const ScanCols& cols,
                            const DictSizes& sizes, const ScanBitmaps& bm, int64_t n_rows, int64_t rows_per_range,
                            int32_t nranges, ColPartial* partials, uint32_t* hll_acc, hipStream_t stream);
hipError_t launch_init_acc(ColPartial* col_acc, int32_t ncol, CorrPartial* pair_acc, int32_t npair, int64_t* rare_dev,
                           hipStream_t st);

#pragma GCC visibility push(hidden)  // (inline helpers: not part of what libdqscan.so exports)

// Preconditions.isNumeric (Analyzer.scala:322-334): ByteType .. DoubleType and DecimalType
inline bool is_numeric(int32_t t) {
  return t == DQ_TYPE_F64 || t == DQ_TYPE_I64 || t == DQ_TYPE_I32 || t == DQ_TYPE_F32 || t == DQ_TYPE_I16 ||
         t == DQ_TYPE_I8 || is_decimal(t);
}
inline bool is_integral(int32_t t) { return t == DQ_TYPE_I64 || t == DQ_TYPE_I32 || t == DQ_TYPE_I16 || t == DQ_TYPE_I8; }
inline bool is_floating(int32_t t) { return t == DQ_TYPE_F64 || t == DQ_TYPE_F32; }
inline bool is_string(int32_t t) { return t == DQ_TYPE_UTF8 || t == DQ_TYPE_LARGE_UTF8; }
inline bool is_dict(int32_t t) { return t == DQ_TYPE_DICT_UTF8; }
// the column types a plan takes: type_valid's, and a dictionary-encoded string column
inline bool plan_type_valid(int32_t t) { return type_valid(t) || is_dict(t); }
inline int32_t kind_of(int32_t t) {
  switch (t) {
    case DQ_TYPE_F64: return CK_F64;
    case DQ_TYPE_I64: case DQ_TYPE_TIMESTAMP: return CK_I64;
    case DQ_TYPE_I32: case DQ_TYPE_DATE32: case DQ_TYPE_DICT_UTF8: return CK_I32;  // (a dictionary column's indices)
    case DQ_TYPE_F32: return CK_F32;
    case DQ_TYPE_I16: return CK_I16;
    case DQ_TYPE_I8: return CK_I8;
    case DQ_TYPE_BOOL: return CK_BOOL;
    case DQ_TYPE_UTF8: return CK_UTF8;
    case DQ_TYPE_LARGE_UTF8: return CK_LUTF8;
    default: return CK_D128;  // (type_valid: a DECIMAL128 code)
  }
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename T>
dq_status dmalloc(T** ptr, size_t bytes) {
  if (bytes == 0) bytes = 16;
  DQ_HIP(hipMalloc((void**)ptr, bytes));
  return DQ_OK;
}

// dq_scan's contract for one column view (dqscan.h dq_column_view)
inline dq_status check_view(const dq_column_desc& cd, const dq_column_view& v, int32_t c, int64_t n_rows) {
  const int32_t t = cd.type;
  if (is_dict(t)) {  // reserved = the number of entries, offsets = the entry words
    if (v.reserved < 0 || v.reserved > INT32_MAX)
      return set_error(DQ_E_INVALID, "dq_scan: dictionary column %d has %lld entries", c, (long long)v.reserved);
    if ((v.reserved > 0 && !v.offsets) || ((uintptr_t)v.offsets & 3) != 0)
      return set_error(DQ_E_INVALID, "dq_scan: dictionary column %d needs a 4-byte aligned entry table", c);
  } else if (v.reserved != 0) return set_error(DQ_E_INVALID, "dq_scan: column %d reserved field must be 0", c);
  if (n_rows > 0 && !v.values) return set_error(DQ_E_INVALID, "dq_scan: column %d has no values buffer", c);
  if (((uintptr_t)v.values & 15) != 0)
    return set_error(DQ_E_INVALID, "dq_scan: column %d values buffer must be 16-byte aligned", c);
  if (((uintptr_t)v.validity & 3) != 0)
    return set_error(DQ_E_INVALID, "dq_scan: column %d validity bitmap must be 4-byte aligned", c);
  if ((t == DQ_TYPE_UTF8 || t == DQ_TYPE_LARGE_UTF8) && n_rows > 0 && !v.offsets)
    return set_error(DQ_E_INVALID, "dq_scan: UTF8 column %d has no offsets", c);
  return DQ_OK;
}

// The kernels' column pointers from the caller's views: the columns `used` marks (null: every column) are checked
// (check_view) and filled; the others' views may be empty and stay null.
inline dq_status fill_scan_cols(const std::vector<dq_column_desc>& schema, const dq_column_view* views, int64_t n_rows,
                                const char* used, ScanCols& sc) {
  for (int32_t c = 0; c < (int32_t)schema.size(); ++c) {
    if (used && !used[c]) continue;
    if (dq_status s = check_view(schema[c], views[c], c, n_rows)) return s;
    sc.values[c] = views[c].values;
    sc.validity[c] = schema[c].nullable ? reinterpret_cast<const uint32_t*>(views[c].validity) : nullptr;
    sc.offsets[c] = views[c].offsets;
  }
  return DQ_OK;
}

// predicate pass (and the row-outcome pass, which must cover the same ranges): ~2048 workgroups of whole 2048-row
// iterations (HBM-bound; counters leave by atomics; 1024-16384 workgroups measured within 2 % on C3)
inline void pred_ranges(int64_t n_rows, int64_t* rows_per_range, int32_t* nranges) {
  const int32_t nr = (int32_t)std::min<int64_t>(
      DQ_PRED_WGS, std::min<int64_t>(ceil_div(n_rows, kRowsPerIter), std::max<int64_t>(1, n_rows / DQ_MIN_RANGE_ROWS)));
  *rows_per_range = ceil_div(ceil_div(n_rows, nr), kRowsPerIter) * kRowsPerIter;
  *nranges = (int32_t)ceil_div(n_rows, *rows_per_range);
}

// dynamic LDS of the interpreter kernels: per wave 128 bytes for every stack level, root and counter, then the DFAs
inline int32_t pred_lds_bytes(const PredProgram& prog) {
  return kWaves * 128 * (prog.stack_depth + prog.n_roots + prog.n_counters) + ((prog.regex_words * 2 + 15) & ~15);
}

// The program and its DFAs to the device, in stream order: the blob into a new *d_regex (when there is one), its
// address into prog.regex, prog into d_prog (allocated by the caller).
inline dq_status upload_pred_program(PredProgram& prog, const std::vector<uint16_t>& regex_blob, uint16_t** d_regex,
                                     PredProgram* d_prog, hipStream_t st) {
  if (!regex_blob.empty()) {
    if (dq_status s = dmalloc(d_regex, regex_blob.size() * sizeof(uint16_t))) return s;
    DQ_HIP(hipMemcpyAsync(*d_regex, regex_blob.data(), regex_blob.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  }
  prog.regex = *d_regex;
  DQ_HIP(hipMemcpyAsync(d_prog, &prog, sizeof(PredProgram), hipMemcpyHostToDevice, st));
  return DQ_OK;
}

#pragma GCC visibility pop

}  // namespace dq
