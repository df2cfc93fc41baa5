// dq_strlen.hip -- the length of every value of a string column as an I32 column with its validity bitmap: what
// MinLength / MaxLength read through the ordinary column scan (Spark computes min(length(col)) the same way, a
// derived expression under an ordinary aggregate).
//
//   dq_utf8_length       UTF8 / LARGE_UTF8 column -> int32 lengths + validity words (the rule: include/dqscan.h)
//   dq_utf8_length_host  the same rule on the CPU, no device (tests)
//   dq_dict_take_i32     out[r] = entry_values[index[r]]: a dictionary column's lengths from its entries' lengths
//
// dq_utf8_length, formulation.  A value's length is its bytes minus its continuation bytes (10xxxxxx).  The kernel is
// built for bytes: wave w of a block takes kGroupsPerWave consecutive 64-row groups; lane l of a group owns row
// base + l, so the offsets are one coalesced load, the lengths one coalesced store and the validity word a ballot.
// The group's values are one contiguous span [off[base], off[base + 64]) of the data buffer.  The wave walks the span
// in 1 KiB chunks, lane l loading the aligned 16 bytes at chunk + 16 l (only 16-byte pieces that hold a byte of the
// span, and no dword past the 4-byte boundary behind the column's last value) -- whatever the rows' lengths, the
// data is read with full-width coalesced loads, once.  Per chunk a row's share is
//     (b - a) - (C(b) - C(a)),   a, b = the row's two offsets clamped into the chunk,
// where C(p) counts the chunk's continuation bytes before byte p.  When the wave-wide OR of the chunk's bytes has no
// high bit -- ASCII, the usual case -- C is 0 and the share is the offset difference alone.  Otherwise each lane
// packs (continuation bytes in the lanes before it) << 16 | (16-bit mask of its own) into one word, the exclusive
// part from a wave prefix sum, and a row reads C(p) with one cross-lane read of lane p / 16's word.  A value longer
// than a chunk, of any length, is simply more trips of the same loop, its row accumulating (64-bit for LARGE_UTF8,
// saturated at INT32_MAX on the store).  Bytes of the chunk outside the span, NULL rows' slots and rows past n_rows
// cancel: only differences of C at offsets inside the span are taken.
//
// Bytes per row: 4 (8) of offsets + the value's bytes + 1/8 of validity in, 4 + 1/8 out.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "dq_hip_host.h"
#include "dq_lane.h"

namespace dq {
namespace {

constexpr int kStrlenBlock = 256;
constexpr int kStrlenGroupsPerWave = 8;                                        // 64-row groups per wave
constexpr int kStrlenRowsPerBlock = kStrlenBlock * kStrlenGroupsPerWave;      // 2048: tests/test_strlen_gpu.py TILE
constexpr int kChunkBytes = 64 * 16;                                           // one 16-byte piece per lane

// bit k of the result: byte k of w is a continuation byte, (b & 0xC0) == 0x80
__host__ __device__ __forceinline__ uint32_t cont_mask4(uint32_t w) {
  const uint32_t m = (w >> 7) & ~(w >> 6) & 0x01010101u;  // bit 0 of each byte
  return ((m * 0x00204081u) >> 21) & 0xFu;                // bits 0, 8, 16, 24 -> 21, 22, 23, 24 (no two products meet)
}

// C(q): continuation bytes of the chunk before its byte q, 0 <= q <= kChunkBytes; pk = this lane's packed word,
// total = C(kChunkBytes).  Every lane of the wave calls it (cross-lane read).
__device__ __forceinline__ uint32_t cont_before(uint32_t pk, uint32_t total, uint32_t q) {
  const uint32_t v = (uint32_t)__shfl((int)pk, (int)((q >> 4) & 63u));
  const uint32_t c = (v >> 16) + (uint32_t)__builtin_popcount(v & ((1u << (q & 15u)) - 1u));
  return q >= (uint32_t)kChunkBytes ? total : c;
}

template <typename OffT>
__global__ __launch_bounds__(kStrlenBlock) void dq_utf8_length_kernel(const uint32_t* __restrict__ data,
                                                                      const OffT* __restrict__ offsets,
                                                                      const uint32_t* validity, int64_t n_rows,
                                                                      int32_t* __restrict__ lengths,
                                                                      uint64_t* __restrict__ out_validity,
                                                                      unsigned long long* null_counter) {
  // byte positions: 64-bit for LARGE_UTF8; unsigned 32-bit for UTF8, whose offsets are below 2^31 (a position plus
  // a chunk cannot wrap)
  using Pos = std::conditional_t<sizeof(OffT) == 8, int64_t, uint32_t>;
  using Acc = std::conditional_t<sizeof(OffT) == 8, int64_t, int32_t>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_groups = (n_rows + 63) >> 6;
  const int64_t g0 = ((int64_t)blockIdx.x * (kStrlenBlock / 64) + wave) * kStrlenGroupsPerWave;
  auto pos = [](OffT o) -> Pos { return o < 0 ? (Pos)0 : (Pos)o; };
  // no dword at or past this byte is read: the data is readable up to the 4-byte boundary behind the last value
  const Pos data_end = (pos(offsets[n_rows]) + 3) & ~(Pos)3;
  uint32_t nulls = 0;  // wave-uniform
  for (int j = 0; j < kStrlenGroupsPerWave; ++j) {
    const int64_t g = g0 + j;
    if (g >= n_groups) break;
    const int64_t base = g * 64;
    const int64_t rows_left = n_rows - base;
    const int32_t left = rows_left < 64 ? (int32_t)rows_left : 64;  // rows of this group, 1..64
    const uint64_t vm = sel_word(validity, base >> 5, left);
    const bool in = lane < left;
    Pos o0 = 0, o1 = 0;
    if (in) {
      o0 = pos(offsets[base + lane]);
      o1 = pos(offsets[base + lane + 1]);
      if (o1 < o0) o1 = o0;
    }
    const Pos first = pos(offsets[base]);  // the group's span [first, last), wave-uniform
    Pos last = pos(offsets[base + left]);
    if (last > data_end) last = data_end;
    Acc len = 0;
    for (Pos lo = first & ~(Pos)15; lo < last; lo += kChunkBytes) {
      const Pos p = lo + 16 * (Pos)lane;  // this lane's piece: bytes [p, p + 16)
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (p < last && p + 16 > first) {
        if (p + 16 <= data_end) {
          const uint4 v = *reinterpret_cast<const uint4*>(data + (p >> 2));
          w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (p + 4 * k < data_end) w[k] = data[(p >> 2) + k];
        }
      }
      const Pos hi = lo + kChunkBytes;
      const Pos ca = o0 < lo ? lo : (o0 > hi ? hi : o0), cb = o1 < lo ? lo : (o1 > hi ? hi : o1);
      const uint32_t a = (uint32_t)(ca - lo), b = (uint32_t)(cb - lo);  // 0 .. kChunkBytes, a <= b
      uint32_t share = b - a;
      const bool high = ((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) != 0u;
      if (__builtin_amdgcn_ballot_w64(high) != 0ull) {  // (wave-uniform) some byte of the chunk is not ASCII
        const uint32_t mask = cont_mask4(w[0]) | cont_mask4(w[1]) << 4 | cont_mask4(w[2]) << 8 | cont_mask4(w[3]) << 12;
        const uint32_t mine = (uint32_t)__builtin_popcount(mask);
        uint32_t incl = mine;  // inclusive prefix sum over the lanes (at most kChunkBytes)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
          if (lane >= d) incl += up;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        const uint32_t pk = (incl - mine) << 16 | mask;
        share -= cont_before(pk, total, b) - cont_before(pk, total, a);
      }
      len += (Acc)share;
    }
    const bool valid = lane_bit(vm);  // (vm is clipped to the group's rows)
    if (!valid) len = 0;
    if (in) lengths[base + lane] = len > (Acc)INT32_MAX ? INT32_MAX : (int32_t)len;
    if (lane == 0) out_validity[g] = vm;
    nulls += (uint32_t)(left - __builtin_popcountll(vm));
  }
  if (null_counter != nullptr && lane == 0 && nulls != 0) atomicAdd(null_counter, (unsigned long long)nulls);
}

// One row per lane, a 64-row group per wave: the index of a row is loaded, and used, only when the row's validity
// bit is set, and addresses entry_values only when it lies inside [0, n_entries).
__global__ __launch_bounds__(kStrlenBlock) void dq_dict_take_i32_kernel(const int32_t* __restrict__ indices,
                                                                        const uint32_t* validity, int64_t n_rows,
                                                                        const int32_t* __restrict__ entry_values,
                                                                        uint32_t n_entries, int32_t* __restrict__ out,
                                                                        uint64_t* __restrict__ out_validity) {
  const int lane = threadIdx.x & 63;
  const int64_t g = ((int64_t)blockIdx.x * kStrlenBlock + threadIdx.x) >> 6;  // wave-uniform
  const int64_t base = g * 64;
  if (base >= n_rows) return;
  const int64_t rows_left = n_rows - base;
  const int32_t left = rows_left < 64 ? (int32_t)rows_left : 64;
  const uint64_t vm = sel_word<true>(validity, base >> 5, left);
  int32_t v = -1;
  if ((vm >> lane) & 1ull) {
    const uint32_t idx = (uint32_t)indices[base + lane];
    if (idx < n_entries) v = entry_values[idx];
  }
  const uint64_t ok = __builtin_amdgcn_ballot_w64(v >= 0);
  if (lane < left) out[base + lane] = v >= 0 ? v : 0;
  if (lane == 0) out_validity[g] = ok;
}

}  // namespace
}  // namespace dq

extern "C" {

dq_status dq_utf8_length(int32_t src_type, const dq_column_view* src, int64_t n_rows, int32_t* lengths,
                         uint64_t* validity_out, int32_t device, void* hip_stream, int64_t* nulls_out) {
  using namespace dq;
  const char* me = "dq_utf8_length";
  if (src_type != DQ_TYPE_UTF8 && src_type != DQ_TYPE_LARGE_UTF8)
    return set_error(DQ_E_UNSUPPORTED, "%s: source type %d is not UTF8 / LARGE_UTF8", me, src_type);
  if (n_rows < 0 || !src || src->reserved != 0) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (nulls_out) *nulls_out = 0;
  if (n_rows == 0) return DQ_OK;
  if (!src->values || !src->offsets || !lengths || !validity_out) return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  const bool large = src_type == DQ_TYPE_LARGE_UTF8;
  if (((uintptr_t)src->values & 15) || ((uintptr_t)src->validity & 3) || ((uintptr_t)src->offsets & (large ? 7 : 3)) ||
      ((uintptr_t)lengths & 3) || ((uintptr_t)validity_out & 7))
    return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
  if (!large && n_rows >= INT32_MAX) return set_error(DQ_E_INVALID, "%s: UTF8 chunk of %lld rows", me, (long long)n_rows);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  StreamBuf counter;  // only when the caller asks for the NULL count (the call then synchronises the stream)
  if (nulls_out) {
    DQ_HIP(counter.alloc(8, st));
    DQ_HIP(hipMemsetAsync(counter.get(), 0, 8, st));
  }
  const unsigned grid = (unsigned)((n_rows + kStrlenRowsPerBlock - 1) / kStrlenRowsPerBlock);
  auto* data = static_cast<const uint32_t*>(src->values);
  auto* val = reinterpret_cast<const uint32_t*>(src->validity);
  auto* cnt = static_cast<unsigned long long*>(counter.get());
  if (large)
    hipLaunchKernelGGL(dq_utf8_length_kernel<int64_t>, dim3(grid), dim3(kStrlenBlock), 0, st, data,
                       static_cast<const int64_t*>(src->offsets), val, n_rows, lengths, validity_out, cnt);
  else
    hipLaunchKernelGGL(dq_utf8_length_kernel<int32_t>, dim3(grid), dim3(kStrlenBlock), 0, st, data,
                       static_cast<const int32_t*>(src->offsets), val, n_rows, lengths, validity_out, cnt);
  DQ_HIP(hipGetLastError());
  if (nulls_out) {
    unsigned long long h = 0;
    DQ_HIP(hipMemcpyAsync(&h, counter.get(), 8, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    *nulls_out = (int64_t)h;
  }
  return DQ_OK;
}

dq_status dq_utf8_length_host(const uint8_t* data, const int64_t* offsets, int64_t n, const uint8_t* validity,
                              int32_t* out) {
  using namespace dq;
  if (n < 0 || (n > 0 && (!offsets || !out))) return set_error(DQ_E_INVALID, "dq_utf8_length_host: bad argument");
  for (int64_t r = 0; r < n; ++r) {
    int64_t len = 0;
    if (!validity || ((validity[r >> 3] >> (r & 7)) & 1))
      for (int64_t p = offsets[r]; p < offsets[r + 1]; ++p) len += (data[p] & 0xC0) != 0x80;
    out[r] = len > INT32_MAX ? INT32_MAX : (int32_t)len;
  }
  return DQ_OK;
}

dq_status dq_dict_take_i32(const dq_column_view* indices, int64_t n_rows, const int32_t* entry_values,
                           int64_t n_entries, int32_t* out, uint64_t* validity_out, int32_t device, void* hip_stream) {
  using namespace dq;
  const char* me = "dq_dict_take_i32";
  if (!indices || n_rows < 0 || n_entries < 0 || n_entries > INT32_MAX) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (n_rows == 0) return DQ_OK;
  if (!indices->values || !out || !validity_out || (n_entries > 0 && !entry_values))
    return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  if (((uintptr_t)indices->values & 3) || ((uintptr_t)indices->validity & 3) || ((uintptr_t)entry_values & 3) ||
      ((uintptr_t)out & 3) || ((uintptr_t)validity_out & 7))
    return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  const unsigned grid = (unsigned)((((n_rows + 63) >> 6) * 64 + kStrlenBlock - 1) / kStrlenBlock);
  hipLaunchKernelGGL(dq_dict_take_i32_kernel, dim3(grid), dim3(kStrlenBlock), 0, st,
                     static_cast<const int32_t*>(indices->values), reinterpret_cast<const uint32_t*>(indices->validity),
                     n_rows, entry_values, (uint32_t)n_entries, out, validity_out);
  DQ_HIP(hipGetLastError());
  return DQ_OK;
}

}  // extern "C"
