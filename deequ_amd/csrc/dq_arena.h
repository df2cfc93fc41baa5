// dq_arena.h -- bookkeeping of the grouping scratch arena (dq_group.hip): per device a list of slots that only grow,
// handed out in sequence to one frame at a time.
//
// A GROUP BY over a 62.5 M-row chunk needs ~2 GB of temporaries, and hipMalloc / hipFree of that much per call costs
// more than the sort itself -- so the blocks stay.  An entry point opens one Frame on its device's list (which
// serialises the calls: the arena is shared by all plans) and passes it down its call chain; every take() gets the
// next slot of the list, so two buffers of one call never share a block, and growing a slot frees only that slot's
// old block, which nobody in the frame holds yet.  Host only, and no HIP: Mem supplies alloc(bytes) -> pointer or
// nullptr, and free(pointer) (DeviceMem in dq_hip_host.h; tests/arena_check.cpp maps them to malloc / free).
#pragma once

#include <algorithm>
#include <cstddef>
#include <map>
#include <mutex>
#include <vector>

namespace dq {

template <typename Mem>
class Arena {
 public:
  struct Slot { void* p = nullptr; size_t cap = 0; };
  class Frame {
   public:
    Frame(Arena& a, int device) : lock_(a.mu_), slots_(a.slots_[device]) {}
    // The frame's next slot, holding at least max(bytes, 256) bytes; nullptr when Mem is exhausted (*want: the size
    // asked of it).  A slot too small is replaced by one of bytes + bytes / 8 (headroom for the next, slightly larger
    // call); its old contents are not kept.
    void* take_bytes(size_t bytes, size_t* want = nullptr) {
      bytes = std::max<size_t>(bytes, 256);
      if (next_ == slots_.size()) slots_.emplace_back();
      Slot& sl = slots_[next_];
      if (sl.cap < bytes) {
        if (sl.p) Mem::free(sl.p);
        sl = Slot{};
        const size_t grown = bytes + bytes / 8;
        if (want) *want = grown;
        sl.p = Mem::alloc(grown);
        if (!sl.p) return nullptr;
        sl.cap = grown;
      }
      ++next_;
      return sl.p;
    }

   private:
    std::lock_guard<std::mutex> lock_;  // (before slots_: the list is looked up under the lock)
    std::vector<Slot>& slots_;
    size_t next_ = 0;
  };

  // what take_bytes() would find (tests)
  size_t num_slots(int device) { return slots_[device].size(); }
  size_t capacity(int device, size_t slot) { return slots_[device][slot].cap; }

 private:
  std::mutex mu_;
  std::map<int, std::vector<Slot>> slots_;
};

}  // namespace dq
