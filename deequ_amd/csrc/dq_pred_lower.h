// dq_pred_lower.h -- predicate lowering (IR tree of dq_pred_node -> postfix PredProgram over three-valued atoms) and
// the one builder of predicate programs, used by the planner (dq_plan.cpp) and by row programs (dq_rowprog.cpp).
// Host only, no HIP runtime call: tests/lower_check.cpp drives it as a stand-alone program.
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "dq_device.h"
#include "dq_internal.h"

namespace dq {

#pragma GCC visibility push(hidden)  // (internal to libdqscan.so: its exports are the C ABI's)

struct Lowering;

// the fixed capacity of a PredProgram a builder call ran into
enum PredLimit { PL_NONE = 0, PL_ROOTS, PL_INSTR, PL_STACK, PL_REGEX };

// Builds one PredProgram: distinct roots (deduplicated by canonical text) in slot order of first use, each root's
// code followed by its STORE.  Counters and `where` bitmaps are the caller's.  A call that fails on a program limit
// returns DQ_E_UNSUPPORTED with `limit` set and words no error: the caller turns it into its own status and
// message.  Every other failure is a lowering error, already worded (set_error).
class PredBuilder {
 public:
  // patterns: the DQ_PRED_REGEX patterns; regex_blob receives their compiled DFAs (dq_regex.h layout)
  PredBuilder(const dq_pred_node* pool, int32_t n_pred, const std::vector<dq_column_desc>* schema,
              const std::vector<std::string>* patterns, std::vector<uint16_t>* regex_blob);
  ~PredBuilder();
  // the slot of the predicate at pool node `node`
  dq_status root(int32_t node, int32_t& slot);
  // the slot of the synthetic root `col IS NOT NULL` (Completeness with a `where`)
  dq_status notnull_root(int32_t col, int32_t& slot);
  int32_t n_roots() const { return (int32_t)root_slot_.size(); }
  // checks the limits and fills prog's regex_words, n_instr, instr, n_roots, stack_depth, n_loads and load_instr
  dq_status assemble(PredProgram& prog);

  PredLimit limit = PL_NONE;
  size_t limit_value = 0;  // PL_ROOTS: kMaxRoots; PL_INSTR: instructions; PL_STACK: stack depth; PL_REGEX: DFA words

 private:
  dq_status over(PredLimit l, size_t value);
  dq_status add(const std::string& key, int32_t node, const PredInstr* atom, int32_t& slot);
  std::unique_ptr<Lowering> low_;
  std::map<std::string, int32_t> root_slot_;  // canonical predicate text (or "notnull:<col>") -> root slot
  std::vector<PredInstr> code_;
};

#pragma GCC visibility pop

}  // namespace dq
