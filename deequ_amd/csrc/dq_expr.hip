// dq_expr.hip -- arithmetic operands of predicates (+ - * / % over numeric columns) materialised as derived columns:
// one postfix dq_expr_program (include/dqscan.h: the Spark 2.2 rules, the instruction set) evaluated over a chunk
// into a column of its result type with a validity bitmap, which the fused scan then reads like any other column.
//
//   dq_expr_eval       the program over up to DQ_EXPR_MAX_COLUMNS device columns -> values + validity words + NULLs
//   dq_expr_eval_host  the same row function on the CPU, no device (tests)
//
// Formulation.  The pass is streaming: per row it reads the inputs' widths plus their validity bits and writes the
// result's width plus one bit.  Lane l of a wave owns row base + l of a 64-row group, so every column is one
// coalesced load, the result one coalesced store and the validity word a ballot; a wave takes kExprGroupsPerWave
// consecutive groups, and again with the grid's stride when the chunk is longer than kExprMaxBlocks workgroups' rows
// (the NULL count is one atomic per wave: with a wave per 256 rows those atomics, all on one address, were the
// whole run time).  All source values of a group are loaded first (independent loads, one wait), then the
// program -- wave-uniform, read with scalar loads from a small device image -- is interpreted once for the 64 rows.
// A value is 64 bits whatever its type: an integral value sign-extended, a float's bits in the low half, a double's
// bits.  The value stack is DQ_EXPR_MAX_STACK named registers that shift on push and pop, so no instruction indexes
// the stack at run time and the kernel uses no scratch memory.  The compiler emitted every cast, so an instruction
// needs only its own type.  Multiplication and addition are separate instructions of separate iterations; the file is
// built with contraction off as well, so a * b + c is never an FMA.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "dq_hip_host.h"
#include "dq_lane.h"

#pragma clang fp contract(off)

namespace dq {
namespace {

constexpr int kExprBlock = 256;
constexpr int kExprGroupsPerWave = 4;                                   // 64-row groups per wave
constexpr int kExprRowsPerBlock = kExprBlock * kExprGroupsPerWave;      // 1024: tests/test_expr_gpu.py TILE
constexpr int kExprMaxBlocks = 2048;  // a longer chunk is walked with a grid stride: one NULL-count atomic per wave

// the device image of a program: what the kernel reads with scalar loads
struct ExprImage {
  uint32_t code[DQ_EXPR_MAX_INSTRS];     // op | arg << 8 | type << 16
  uint64_t lits[DQ_EXPR_MAX_LITERALS];   // the literal as a stack value
};

struct ExprCols {
  const void* values[DQ_EXPR_MAX_COLUMNS];
  const uint32_t* validity[DQ_EXPR_MAX_COLUMNS];
  int32_t size[DQ_EXPR_MAX_COLUMNS];  // bytes per element: 1, 2, 4, 8
  int32_t n_cols;
};

__host__ __device__ __forceinline__ bool is_integral(int32_t t) {
  return t == DQ_TYPE_I8 || t == DQ_TYPE_I16 || t == DQ_TYPE_I32 || t == DQ_TYPE_I64;
}
__host__ __device__ __forceinline__ int32_t type_size(int32_t t) {
  switch (t) {
    case DQ_TYPE_I8: return 1;
    case DQ_TYPE_I16: return 2;
    case DQ_TYPE_I32: case DQ_TYPE_F32: return 4;
    case DQ_TYPE_I64: case DQ_TYPE_F64: return 8;
    default: return 0;
  }
}
__host__ __device__ __forceinline__ float as_f32(uint64_t v) { return __builtin_bit_cast(float, (uint32_t)v); }
__host__ __device__ __forceinline__ double as_f64(uint64_t v) { return __builtin_bit_cast(double, v); }
__host__ __device__ __forceinline__ uint64_t of_f32(float f) { return (uint64_t)__builtin_bit_cast(uint32_t, f); }
__host__ __device__ __forceinline__ uint64_t of_f64(double d) { return __builtin_bit_cast(uint64_t, d); }

// two's-complement wrap of an integral result at the width of `type`, sign-extended again
__host__ __device__ __forceinline__ uint64_t wrap_to(uint64_t r, int32_t type) {
  switch (type) {
    case DQ_TYPE_I8: return (uint64_t)(int64_t)(int8_t)(uint8_t)r;
    case DQ_TYPE_I16: return (uint64_t)(int64_t)(int16_t)(uint16_t)r;
    case DQ_TYPE_I32: return (uint64_t)(int64_t)(int32_t)(uint32_t)r;
    default: return r;
  }
}

// CAST of a stack value whose type is integral (from_int) or F32 to the wider `type`
__host__ __device__ __forceinline__ uint64_t cast_to(uint64_t v, bool from_int, int32_t type) {
  if (type == DQ_TYPE_F32) return of_f32((float)(int64_t)v);                       // integral -> Float, one rounding
  if (type == DQ_TYPE_F64) return of_f64(from_int ? (double)(int64_t)v : (double)as_f32(v));
  return v;                                                                          // integral -> wider integral
}

__host__ __device__ __forceinline__ uint64_t negate(uint64_t v, int32_t type) {
  if (type == DQ_TYPE_F32) return v ^ 0x80000000ull;
  if (type == DQ_TYPE_F64) return v ^ 0x8000000000000000ull;
  return wrap_to(0ull - v, type);
}

// a op b at `type` (DIV: F64); ok is cleared where the rules give NULL (a zero divisor of / or %)
__host__ __device__ __forceinline__ uint64_t binary(int32_t op, int32_t type, uint64_t a, uint64_t b, bool& ok) {
  if (type == DQ_TYPE_F64) {
    const double x = as_f64(a), y = as_f64(b);
    switch (op) {
      case DQ_EXPR_ADD: return of_f64(x + y);
      case DQ_EXPR_SUB: return of_f64(x - y);
      case DQ_EXPR_MUL: return of_f64(x * y);
      case DQ_EXPR_DIV:
        if (y == 0.0) ok = false;
        return of_f64(x / (y == 0.0 ? 1.0 : y));
      default:
        if (y == 0.0) ok = false;
        return of_f64(fmod(x, y == 0.0 ? 1.0 : y));
    }
  }
  if (type == DQ_TYPE_F32) {
    const float x = as_f32(a), y = as_f32(b);
    switch (op) {
      case DQ_EXPR_ADD: return of_f32(x + y);
      case DQ_EXPR_SUB: return of_f32(x - y);
      case DQ_EXPR_MUL: return of_f32(x * y);
      default:
        if (y == 0.0f) ok = false;
        return of_f32(fmodf(x, y == 0.0f ? 1.0f : y));
    }
  }
  switch (op) {
    case DQ_EXPR_ADD: return wrap_to(a + b, type);
    case DQ_EXPR_SUB: return wrap_to(a - b, type);
    case DQ_EXPR_MUL: return wrap_to(a * b, type);
    default: {  // Java's truncated remainder; MIN % -1 is 0 (and has no trap to avoid elsewhere)
      if (b == 0) ok = false;
      if (b == 0 || (int64_t)b == -1) return 0;
      if (type == DQ_TYPE_I64) return (uint64_t)((int64_t)a % (int64_t)b);
      return (uint64_t)(int64_t)((int32_t)(int64_t)a % (int32_t)(int64_t)b);
    }
  }
}

// One row (device: one row per lane, the program wave-uniform).  code / lits: the image; col(k): the value of
// program column k as a stack value.  Returns the result; ok is cleared where it is NULL by the rules.
template <typename Code, typename Lits, typename Col>
__host__ __device__ __forceinline__ uint64_t run_program(Code code, Lits lits, int32_t n_instrs, Col&& col, bool& ok) {
  static_assert(DQ_EXPR_MAX_STACK == 8, "the stack registers below are written out for 8 entries");
  uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
  for (int32_t pc = 0; pc < n_instrs; ++pc) {
    const uint32_t w = code[pc];
    const int32_t op = (int32_t)(w & 0xFFu), arg = (int32_t)((w >> 8) & 0xFFu), type = (int32_t)((w >> 16) & 0xFFu);
    if (op == DQ_EXPR_COL || op == DQ_EXPR_LIT) {
      const uint64_t v = op == DQ_EXPR_COL ? col(arg) : (uint64_t)lits[arg];
      s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
    } else if (op == DQ_EXPR_CAST) {
      s0 = cast_to(s0, (w >> 24) != 0u, type);
    } else if (op == DQ_EXPR_NEG) {
      s0 = negate(s0, type);
    } else {
      s0 = binary(op, type, s1, s0, ok);
      s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
    }
  }
  return s0;
}

__global__ __launch_bounds__(kExprBlock) void dq_expr_kernel(const ExprCols cols, const ExprImage* __restrict__ image,
                                                             int32_t n_instrs, int32_t out_size, int64_t n_rows,
                                                             void* __restrict__ out, uint64_t* __restrict__ out_validity,
                                                             unsigned long long* null_counter) {
  typedef const __attribute__((address_space(4))) uint64_t* const_u64s;
  const const_u32s code = (const_u32s)image->code;
  const const_u64s lits = (const_u64s)image->lits;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_groups = (n_rows + 63) >> 6;
  const int64_t stride = (int64_t)gridDim.x * (kExprBlock / 64) * kExprGroupsPerWave;
  uint32_t nulls = 0;  // wave-uniform
  for (int64_t g0 = ((int64_t)blockIdx.x * (kExprBlock / 64) + wave) * kExprGroupsPerWave; g0 < n_groups; g0 += stride)
  for (int j = 0; j < kExprGroupsPerWave; ++j) {
    const int64_t g = g0 + j;
    if (g >= n_groups) break;
    const int64_t base = g * 64;
    const int64_t rows_left = n_rows - base;
    const int32_t left = rows_left < 64 ? (int32_t)rows_left : 64;  // rows of this group, 1..64
    const bool in = lane < left;
    const int64_t row = base + lane;
    uint64_t vm = left < 64 ? (1ull << left) - 1ull : ~0ull;  // rows whose every input is valid
    uint64_t c[DQ_EXPR_MAX_COLUMNS];
#pragma unroll
    for (int k = 0; k < DQ_EXPR_MAX_COLUMNS; ++k) {
      c[k] = 0;
      if (k < cols.n_cols) {  // (wave-uniform)
        vm &= sel_word(cols.validity[k], base >> 5, left);
        if (in) {  // only rows below n_rows are read
          const int32_t sz = cols.size[k];
          if (sz == 8) c[k] = static_cast<const uint64_t*>(cols.values[k])[row];
          else if (sz == 4) c[k] = (uint64_t)(int64_t) static_cast<const int32_t*>(cols.values[k])[row];
          else if (sz == 2) c[k] = (uint64_t)(int64_t) static_cast<const int16_t*>(cols.values[k])[row];
          else c[k] = (uint64_t)(int64_t) static_cast<const int8_t*>(cols.values[k])[row];
        }
      }
    }
    bool ok = true;
    const uint64_t r = run_program(code, lits, n_instrs, [&](int32_t k) -> uint64_t {
      switch (k) {
        case 0: return c[0];
        case 1: return c[1];
        case 2: return c[2];
        case 3: return c[3];
        case 4: return c[4];
        case 5: return c[5];
        case 6: return c[6];
        default: return c[7];
      }
    }, ok);
    const uint64_t valid = __builtin_amdgcn_ballot_w64(ok) & vm;  // (vm is clipped to the group's rows)
    const uint64_t v = lane_bit(valid) ? r : 0ull;
    if (in) {
      if (out_size == 8) static_cast<uint64_t*>(out)[row] = v;
      else if (out_size == 4) static_cast<uint32_t*>(out)[row] = (uint32_t)v;
      else if (out_size == 2) static_cast<uint16_t*>(out)[row] = (uint16_t)v;
      else static_cast<uint8_t*>(out)[row] = (uint8_t)v;
    }
    if (lane == 0) out_validity[g] = valid;
    nulls += (uint32_t)(left - __builtin_popcountll(valid));
  }
  if (lane == 0 && nulls != 0) atomicAdd(null_counter, (unsigned long long)nulls);
}

// The program as the evaluators take it, after every check a caller's struct needs: limits, indices, the stack
// discipline and the type of every operand.  CAST instructions get bit 24 of their word when they widen an
// integral value (the evaluators do not track types).
dq_status check_and_pack(const char* me, const dq_expr_program* p, ExprImage* img) {
  if (!p) return set_error(DQ_E_INVALID, "%s: NULL program", me);
  if (p->n_instrs < 1 || p->n_instrs > DQ_EXPR_MAX_INSTRS || p->n_columns < 1 || p->n_columns > DQ_EXPR_MAX_COLUMNS ||
      p->n_literals < 0 || p->n_literals > DQ_EXPR_MAX_LITERALS)
    return set_error(DQ_E_INVALID, "%s: program outside the limits (%d instructions, %d columns, %d literals)", me,
                     p->n_instrs, p->n_columns, p->n_literals);
  for (int32_t k = 0; k < p->n_columns; ++k)
    if (!type_size(p->column_types[k]))
      return set_error(DQ_E_UNSUPPORTED, "%s: column %d has type %d, not one of I8 I16 I32 I64 F32 F64", me, k,
                       p->column_types[k]);
  if (!type_size(p->result_type))
    return set_error(DQ_E_UNSUPPORTED, "%s: result type %d is not one of I8 I16 I32 I64 F32 F64", me, p->result_type);
  std::memset(img, 0, sizeof(*img));
  for (int32_t k = 0; k < p->n_literals; ++k) {
    const dq_expr_literal& l = p->literals[k];
    if (l.type == DQ_TYPE_F64) img->lits[k] = of_f64(l.f64);
    else if (l.type == DQ_TYPE_I64 || (l.type == DQ_TYPE_I32 && l.i64 >= INT32_MIN && l.i64 <= INT32_MAX))
      img->lits[k] = (uint64_t)l.i64;
    else return set_error(DQ_E_INVALID, "%s: literal %d has type %d or a value outside it", me, k, l.type);
  }
  int32_t stack[DQ_EXPR_MAX_STACK];
  int32_t depth = 0;
  auto rank = [](int32_t t) { return t == DQ_TYPE_F64 ? 6 : t == DQ_TYPE_F32 ? 5 : type_size(t) == 8 ? 4 : type_size(t) == 4 ? 3 : type_size(t); };
  for (int32_t i = 0; i < p->n_instrs; ++i) {
    const dq_expr_instr& x = p->instrs[i];
    uint32_t flag = 0;
    bool good = type_size(x.type) != 0;
    switch (x.op) {
      case DQ_EXPR_COL:
        good = good && x.arg >= 0 && x.arg < p->n_columns && x.type == p->column_types[x.arg] && depth < DQ_EXPR_MAX_STACK;
        if (good) stack[depth++] = x.type;
        break;
      case DQ_EXPR_LIT:
        good = good && x.arg >= 0 && x.arg < p->n_literals && x.type == p->literals[x.arg].type && depth < DQ_EXPR_MAX_STACK;
        if (good) stack[depth++] = x.type;
        break;
      case DQ_EXPR_CAST:
        good = good && depth >= 1 && rank(x.type) > rank(stack[depth - 1]);
        if (good) {
          flag = is_integral(stack[depth - 1]) ? 1u : 0u;
          stack[depth - 1] = x.type;
        }
        break;
      case DQ_EXPR_NEG:
        good = good && depth >= 1 && stack[depth - 1] == x.type;
        break;
      case DQ_EXPR_ADD: case DQ_EXPR_SUB: case DQ_EXPR_MUL: case DQ_EXPR_DIV: case DQ_EXPR_MOD:
        good = good && depth >= 2 && stack[depth - 1] == x.type && stack[depth - 2] == x.type &&
               (x.op != DQ_EXPR_DIV || x.type == DQ_TYPE_F64);
        if (good) --depth;
        break;
      default: good = false;
    }
    if (!good) return set_error(DQ_E_INVALID, "%s: instruction %d (op %d, arg %d, type %d) is malformed", me, i, x.op, x.arg, x.type);
    img->code[i] = (uint32_t)x.op | (uint32_t)x.arg << 8 | (uint32_t)x.type << 16 | flag << 24;
  }
  if (depth != 1 || stack[0] != p->result_type)
    return set_error(DQ_E_INVALID, "%s: the program leaves %d values, the last of type %d, not one of type %d", me,
                     depth, depth ? stack[depth - 1] : 0, p->result_type);
  return DQ_OK;
}

}  // namespace
}  // namespace dq

extern "C" {

dq_status dq_expr_eval(const dq_expr_program* prog, const dq_column_view* cols, int64_t n_rows, void* out_values,
                       uint64_t* out_validity, int32_t device, void* hip_stream, int64_t* nulls_out) {
  using namespace dq;
  const char* me = "dq_expr_eval";
  ExprImage img;
  if (dq_status s = check_and_pack(me, prog, &img)) return s;
  if (n_rows < 0 || !cols) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  ExprCols dc{};
  dc.n_cols = prog->n_columns;
  for (int32_t k = 0; k < prog->n_columns; ++k) {
    if (cols[k].reserved != 0) return set_error(DQ_E_INVALID, "%s: column %d: reserved must be 0", me, k);
    if (n_rows > 0 && !cols[k].values) return set_error(DQ_E_INVALID, "%s: column %d: NULL buffer", me, k);
    if (((uintptr_t)cols[k].values & 15) || ((uintptr_t)cols[k].validity & 3))
      return set_error(DQ_E_INVALID, "%s: column %d: misaligned buffer", me, k);
    dc.values[k] = cols[k].values;
    dc.validity[k] = reinterpret_cast<const uint32_t*>(cols[k].validity);
    dc.size[k] = type_size(prog->column_types[k]);
  }
  if (nulls_out) *nulls_out = 0;
  if (n_rows == 0) return DQ_OK;
  if (!out_values || !out_validity) return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  if (((uintptr_t)out_values & 15) || ((uintptr_t)out_validity & 7)) return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
  const int64_t blocks = (n_rows + kExprRowsPerBlock - 1) / kExprRowsPerBlock;
  const unsigned grid = (unsigned)(blocks < kExprMaxBlocks ? blocks : kExprMaxBlocks);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  // one temporary: the NULL counter, then the program image (the call synchronises, so `img` outlives the copy)
  StreamBuf tmp;
  DQ_HIP(tmp.alloc(16 + sizeof(ExprImage), st));
  auto* counter = static_cast<unsigned long long*>(tmp.get());
  auto* image = reinterpret_cast<ExprImage*>(static_cast<char*>(tmp.get()) + 16);
  DQ_HIP(hipMemsetAsync(counter, 0, 16, st));
  DQ_HIP(hipMemcpyAsync(image, &img, sizeof(img), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dq_expr_kernel, dim3(grid), dim3(kExprBlock), 0, st, dc, image, prog->n_instrs,
                     type_size(prog->result_type), n_rows, out_values, out_validity, counter);
  DQ_HIP(hipGetLastError());
  unsigned long long h = 0;
  DQ_HIP(hipMemcpyAsync(&h, counter, 8, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (nulls_out) *nulls_out = (int64_t)h;
  return DQ_OK;
}

dq_status dq_expr_eval_host(const dq_expr_program* prog, const dq_column_view* cols, int64_t n_rows, void* out_values,
                            uint64_t* out_validity, int64_t* nulls_out) {
  using namespace dq;
  const char* me = "dq_expr_eval_host";
  ExprImage img;
  if (dq_status s = check_and_pack(me, prog, &img)) return s;
  if (n_rows < 0 || !cols || (n_rows > 0 && (!out_values || !out_validity)))
    return set_error(DQ_E_INVALID, "%s: bad argument", me);
  for (int32_t k = 0; k < prog->n_columns; ++k)
    if (n_rows > 0 && !cols[k].values) return set_error(DQ_E_INVALID, "%s: column %d: NULL buffer", me, k);
  const int32_t out_size = type_size(prog->result_type);
  int64_t nulls = 0;
  for (int64_t w = 0; w < (n_rows + 63) / 64; ++w) out_validity[w] = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    bool ok = true;
    for (int32_t k = 0; k < prog->n_columns; ++k)
      if (cols[k].validity && !((cols[k].validity[r >> 3] >> (r & 7)) & 1)) ok = false;
    uint64_t v = run_program(img.code, img.lits, prog->n_instrs, [&](int32_t k) -> uint64_t {
      const char* p = static_cast<const char*>(cols[k].values);
      switch (type_size(prog->column_types[k])) {
        case 8: { int64_t x; std::memcpy(&x, p + 8 * r, 8); return (uint64_t)x; }
        case 4: { int32_t x; std::memcpy(&x, p + 4 * r, 4); return (uint64_t)(int64_t)x; }
        case 2: { int16_t x; std::memcpy(&x, p + 2 * r, 2); return (uint64_t)(int64_t)x; }
        default: { int8_t x; std::memcpy(&x, p + r, 1); return (uint64_t)(int64_t)x; }
      }
    }, ok);
    if (!ok) v = 0, ++nulls;
    else out_validity[r >> 6] |= 1ull << (r & 63);
    std::memcpy(static_cast<char*>(out_values) + (int64_t)out_size * r, &v, (size_t)out_size);  // (little-endian)
  }
  if (nulls_out) *nulls_out = nulls;
  return DQ_OK;
}

}  // extern "C"
