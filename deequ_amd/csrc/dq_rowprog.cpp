// dq_rowprog.cpp -- row programs (dq_row_outcomes): a predicate program whose "counters" are its outputs --
// prog.counters[k] holds output k's (predicate, where) root slots -- run by dq_row_outcomes_scan (dq_kernels.hip),
// which stores the rows' outcomes where dq_pred_scan counts them.  Lowered on the host at creation (no device, by
// the planner's builder: dq_pred_lower.h); the program, its DFAs and the count accumulators go to the device of the
// first evaluation.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dq_plan_host.h"
#include "dq_pred_lower.h"

using namespace dq;

struct dq_row_program {
  std::vector<dq_column_desc> schema;
  std::vector<std::string> patterns;
  std::vector<uint16_t> regex_blob;
  PredProgram prog{};
  int32_t device = -1;  // where d_prog / d_regex / d_acc live (-1: nowhere yet)
  PredProgram* d_prog = nullptr;
  uint16_t* d_regex = nullptr;
  PredPartial* d_acc = nullptr;
};

static void row_program_free_device(dq_row_program* rp) {
  if (rp->device < 0) return;
  (void)hipSetDevice(rp->device);
  if (rp->d_prog) (void)hipFree(rp->d_prog);
  if (rp->d_regex) (void)hipFree(rp->d_regex);
  if (rp->d_acc) (void)hipFree(rp->d_acc);
  rp->d_prog = nullptr;
  rp->d_regex = nullptr;
  rp->d_acc = nullptr;
  rp->device = -1;
}

static dq_status row_program_build(dq_row_program* rp, const dq_pred_node* pool, int32_t n_pred,
                                   const dq_row_output* outputs, int32_t n_out) {
  PredBuilder pb(pool, n_pred, &rp->schema, &rp->patterns, &rp->regex_blob);
  // a program limit is the caller's to split around (rowlevel.plan_row_level): never the capacity flag
  auto refused = [&](dq_status s) -> dq_status {
    switch (pb.limit) {
      case PL_ROOTS:
        return set_error(DQ_E_UNSUPPORTED, "dq_row_program_create: more than %d distinct roots (split the outputs)", kMaxRoots);
      case PL_INSTR:
        return set_error(DQ_E_UNSUPPORTED, "dq_row_program_create: program too long (%zu instructions, at most %d: split the outputs)",
                         pb.limit_value, kMaxInstr);
      case PL_STACK:
        return set_error(DQ_E_UNSUPPORTED, "predicate nesting needs a stack of %d (at most %d)", (int)pb.limit_value, kPredStack);
      case PL_REGEX:
        return set_error(DQ_E_UNSUPPORTED, "dq_row_program_create: compiled patterns need %zu KB (LDS budget %d KB: split the outputs)",
                         pb.limit_value * 2 / 1024, kMaxRegexWords * 2 / 1024);
      default: return s;
    }
  };
  PredProgram& prog = rp->prog;
  std::memset(&prog, 0, sizeof(prog));
  for (int32_t k = 0; k < n_out; ++k) {
    int32_t ps = -1, ws = -1;
    if (dq_status s = refused(pb.root(outputs[k].pred_root, ps))) return s;
    if (outputs[k].where_root >= 0)
      if (dq_status s = refused(pb.root(outputs[k].where_root, ws))) return s;
    prog.counters[k] = PredCounter{ps, ws};
  }
  if (dq_status s = refused(pb.assemble(prog))) return s;
  prog.n_counters = n_out;
  return DQ_OK;
}

extern "C" {

int32_t dq_row_max_outputs(void) { return kMaxRoots; }

dq_status dq_row_program_create(const dq_column_desc* schema, int32_t n_cols, const dq_pred_node* pred_pool,
                                int32_t n_pred, const char* const* patterns, int32_t n_patterns,
                                const dq_row_output* outputs, int32_t n_out, dq_row_program** out) {
  if (!out) return set_error(DQ_E_INVALID, "dq_row_program_create: out is NULL");
  *out = nullptr;
  if (n_cols < 0 || (n_cols > 0 && !schema)) return set_error(DQ_E_INVALID, "dq_row_program_create: bad schema");
  if (n_cols > kMaxCols)
    return set_error(DQ_E_UNSUPPORTED, "dq_row_program_create: more than %d columns (pass the columns the outputs read)", kMaxCols);
  if (n_pred < 0 || (n_pred > 0 && !pred_pool)) return set_error(DQ_E_INVALID, "dq_row_program_create: bad predicate pool");
  if (n_patterns < 0 || (n_patterns > 0 && !patterns)) return set_error(DQ_E_INVALID, "dq_row_program_create: bad patterns");
  for (int32_t k = 0; k < n_patterns; ++k)
    if (!patterns[k]) return set_error(DQ_E_INVALID, "dq_row_program_create: pattern %d is NULL", k);
  if (n_out < 1 || !outputs) return set_error(DQ_E_INVALID, "dq_row_program_create: no outputs");
  if (n_out > kMaxCounters)
    return set_error(DQ_E_UNSUPPORTED, "dq_row_program_create: more than %d outputs (split them)", kMaxCounters);
  for (int32_t c = 0; c < n_cols; ++c)
    if (!plan_type_valid(schema[c].type))
      return set_error(DQ_E_TYPE, "dq_row_program_create: column %d has unknown type %d", c, schema[c].type);
  std::unique_ptr<dq_row_program> rp(new dq_row_program());
  rp->schema.assign(schema, schema + n_cols);
  for (int32_t k = 0; k < n_patterns; ++k) rp->patterns.emplace_back(patterns[k]);
  if (dq_status s = row_program_build(rp.get(), pred_pool, n_pred, outputs, n_out)) return s;
  *out = rp.release();
  return DQ_OK;
}

dq_status dq_row_program_info(const dq_row_program* rp, int32_t* n_outputs, int32_t* n_roots, int32_t* n_instr) {
  if (!rp) return set_error(DQ_E_INVALID, "dq_row_program_info: program is NULL");
  if (n_outputs) *n_outputs = rp->prog.n_counters;
  if (n_roots) *n_roots = rp->prog.n_roots;
  if (n_instr) *n_instr = rp->prog.n_instr;
  return DQ_OK;
}

void dq_row_program_destroy(dq_row_program* rp) {
  if (!rp) return;
  row_program_free_device(rp);
  delete rp;
}

dq_status dq_row_outcomes(dq_row_program* rp, const dq_column_view* cols, int64_t n_rows, uint64_t* const* pass,
                          uint64_t* const* applies, int32_t device, void* hip_stream, int64_t* num_pass,
                          int64_t* num_applies) {
  if (!rp) return set_error(DQ_E_INVALID, "dq_row_outcomes: program is NULL");
  if (n_rows < 0) return set_error(DQ_E_INVALID, "dq_row_outcomes: n_rows < 0");
  if (n_rows >= (int64_t(1) << 31))
    return set_error(DQ_E_INVALID, "dq_row_outcomes: a chunk holds at most 2^31 - 1 rows (split larger inputs into chunks)");
  const int32_t ncols = (int32_t)rp->schema.size(), n_out = rp->prog.n_counters;
  if (n_rows == 0) {
    for (int32_t k = 0; k < n_out; ++k) {
      if (num_pass) num_pass[k] = 0;
      if (num_applies) num_applies[k] = 0;
    }
    return DQ_OK;
  }
  if (ncols > 0 && !cols) return set_error(DQ_E_INVALID, "dq_row_outcomes: cols is NULL");
  if (!pass) return set_error(DQ_E_INVALID, "dq_row_outcomes: pass is NULL");
  for (int32_t k = 0; k < n_out; ++k) {
    if (!pass[k] || ((uintptr_t)pass[k] & 7) != 0)
      return set_error(DQ_E_INVALID, "dq_row_outcomes: pass[%d] must be an 8-byte aligned device buffer", k);
    if (applies && ((uintptr_t)applies[k] & 7) != 0)
      return set_error(DQ_E_INVALID, "dq_row_outcomes: applies[%d] must be 8-byte aligned", k);
  }
  // the columns the program reads (the others' views may be empty)
  std::vector<char> used(ncols, 0);
  for (int32_t i = 0; i < rp->prog.n_instr; ++i) {
    if (rp->prog.instr[i].col_a >= 0) used[rp->prog.instr[i].col_a] = 1;
    if (rp->prog.instr[i].col_b >= 0) used[rp->prog.instr[i].col_b] = 1;
  }
  ScanCols sc{};
  if (dq_status s = fill_scan_cols(rp->schema, cols, n_rows, used.data(), sc)) return s;
  int ndev = 0;
  DQ_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return set_error(DQ_E_INVALID, "dq_row_outcomes: device %d of %d", device, ndev);
  const hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  if (rp->device != device) {
    row_program_free_device(rp);
    DQ_HIP(hipSetDevice(device));
    rp->device = device;
    if (dq_status s = dmalloc(&rp->d_prog, sizeof(PredProgram))) return s;
    if (dq_status s = dmalloc(&rp->d_acc, kPredAccCopies * sizeof(PredPartial))) return s;
    if (dq_status s = upload_pred_program(rp->prog, rp->regex_blob, &rp->d_regex, rp->d_prog, st)) return s;
  }
  DQ_HIP(hipSetDevice(device));
  int32_t nr;
  int64_t rpr;
  pred_ranges(n_rows, &rpr, &nr);  // (dq_scan's predicate-pass ranges)
  DQ_HIP(hipMemsetAsync(rp->d_acc, 0, kPredAccCopies * sizeof(PredPartial), st));
  DQ_HIP(launch_row_outcomes(rp->d_prog, sc, reinterpret_cast<uint32_t* const*>(pass),
                             reinterpret_cast<uint32_t* const*>(applies), n_out, n_rows, rpr, nr, rp->d_acc,
                             pred_lds_bytes(rp->prog), st, rp->prog.regex_words > 0));
  std::vector<PredPartial> acc(kPredAccCopies);
  DQ_HIP(hipMemcpyAsync(acc.data(), rp->d_acc, kPredAccCopies * sizeof(PredPartial), hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  for (int32_t k = 0; k < n_out; ++k) {
    int64_t t = 0, a = 0;
    for (int c = 0; c < kPredAccCopies; ++c) { t += acc[c].t[k]; a += acc[c].nn[k]; }
    if (num_pass) num_pass[k] = t;
    if (num_applies) num_applies[k] = a;
  }
  return DQ_OK;
}

}  // extern "C"
