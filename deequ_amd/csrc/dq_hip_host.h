// dq_hip_host.h -- the host side's HIP plumbing, one copy for every translation unit: the error macro, the owner of
// hipMalloc'ed memory, the owner of a stream-ordered temporary, and the device memory hooks of dq_arena.h.
#pragma once

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

#include <hip/hip_runtime.h>

#include "dq_internal.h"

// A failed HIP call ends the calling function with the library's status: DQ_E_OOM when the device is out of memory
// ("device allocation failed", dqscan.h), DQ_E_HIP for everything else.
#define DQ_HIP(call)                                                                                            \
  do {                                                                                                          \
    const hipError_t dq_hip_e_ = (call);                                                                        \
    if (dq_hip_e_ != hipSuccess)                                                                                \
      return ::dq::set_error(dq_hip_e_ == hipErrorOutOfMemory ? DQ_E_OOM : DQ_E_HIP, "%s: %s failed: %s (%s:%d)", \
                             __func__, #call, hipGetErrorString(dq_hip_e_), __FILE__, __LINE__);                \
  } while (0)

namespace dq {

// owner of one hipMalloc'ed array of T (void: bytes), freed with it; move-only
template <typename T = void>
class DevPtr {
 public:
  DevPtr() = default;
  DevPtr(DevPtr&& o) noexcept : p_(o.release()) {}
  DevPtr& operator=(DevPtr&& o) noexcept {
    if (this != &o) reset(), p_ = o.release();
    return *this;
  }
  ~DevPtr() { reset(); }
  hipError_t alloc(size_t count) {
    reset();
    return hipMalloc(reinterpret_cast<void**>(&p_), count * sizeof(std::conditional_t<std::is_void_v<T>, char, T>));
  }
  T* get() const { return p_; }
  template <typename U> U* as() const { return reinterpret_cast<U*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  T* release() { return std::exchange(p_, nullptr); }

 private:
  T* p_ = nullptr;
};

// owner of one stream-ordered temporary (at least 16 bytes): from the device's default pool or from a pool of the
// library's own, returned in stream order -- also before a second alloc() takes the next block
class StreamBuf {
 public:
  StreamBuf() = default;
  StreamBuf(const StreamBuf&) = delete;
  StreamBuf& operator=(const StreamBuf&) = delete;
  ~StreamBuf() { reset(); }
  hipError_t alloc(size_t bytes, hipStream_t st) {
    reset();
    s_ = st;
    return hipMallocAsync(&p_, std::max<size_t>(bytes, 16), st);
  }
  hipError_t alloc(size_t bytes, hipMemPool_t pool, hipStream_t st) {
    reset();
    s_ = st;
    return hipMallocFromPoolAsync(&p_, std::max<size_t>(bytes, 16), pool, st);
  }
  void* get() const { return p_; }
  void reset() {
    if (p_) (void)hipFreeAsync(p_, s_);
    p_ = nullptr;
  }

 private:
  void* p_ = nullptr;
  hipStream_t s_ = nullptr;
};

// dq_arena.h's memory hooks for the current device
struct DeviceMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
  }
  static void free(void* p) { (void)hipFree(p); }
};

}  // namespace dq
