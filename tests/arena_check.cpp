// arena_check.cpp -- the slot bookkeeping of the grouping scratch arena (deequ_amd/csrc/dq_arena.h) on the host: the
// memory hooks are malloc / free with their calls counted.  A stand-alone program (tests/test_arena_host.py builds it
// with g++ under ASan + UBSan and runs it); nothing here touches HIP.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "dq_arena.h"

namespace {

int g_allocs = 0, g_frees = 0;
size_t g_last_alloc = 0;
struct HostMem {
  static void* alloc(size_t bytes) {
    ++g_allocs;
    g_last_alloc = bytes;
    return std::malloc(bytes);
  }
  static void free(void* p) {
    ++g_frees;
    std::free(p);
  }
};
using Arena = dq::Arena<HostMem>;
using Frame = Arena::Frame;

int g_checks = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++g_checks;                                                          \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

struct Taken {
  unsigned char* p;
  size_t bytes;
  unsigned char fill;
};

Taken take(Frame& f, std::vector<Taken>& live, size_t bytes) {
  Taken t{static_cast<unsigned char*>(f.take_bytes(bytes)), bytes, (unsigned char)(0x11 * (live.size() + 1))};
  CHECK(t.p != nullptr);
  std::memset(t.p, t.fill, bytes);  // (ASan: the whole request is writable)
  live.push_back(t);
  return t;
}

// pairwise disjoint, and every buffer still holds its own fill
void check_live(const std::vector<Taken>& live) {
  for (size_t i = 0; i < live.size(); ++i) {
    for (size_t k = 0; k < live[i].bytes; ++k) CHECK(live[i].p[k] == live[i].fill);
    for (size_t j = i + 1; j < live.size(); ++j)
      CHECK(live[i].p + live[i].bytes <= live[j].p || live[j].p + live[j].bytes <= live[i].p);
  }
}

// a helper deep in a call chain: takes two buffers of its own while the caller's are live
void nested_helper(Frame& f, std::vector<Taken>& live, size_t bytes) {
  take(f, live, bytes);
  take(f, live, 3 * bytes);
  check_live(live);
}

}  // namespace

int main() {
  static Arena& arena = *new Arena;  // (never destroyed: its blocks stay reachable, as the library's global's do)
  // 1. one frame: buffers are pairwise disjoint, a nested helper's included; the growth rule
  {
    Frame f(arena, 0);
    std::vector<Taken> live;
    take(f, live, 1);  // the 256-byte floor, then bytes + bytes / 8
    CHECK(g_allocs == 1 && g_last_alloc == 256 + 256 / 8);
    take(f, live, 1000);
    CHECK(g_allocs == 2 && g_last_alloc == 1000 + 1000 / 8);
    take(f, live, 4096);
    nested_helper(f, live, 700);
    take(f, live, 64);
    check_live(live);
    CHECK(g_allocs == 6 && g_frees == 0 && arena.num_slots(0) == 6);
  }
  const size_t caps[6] = {288, 1125, 4608, 787, 2362, 288};
  for (int i = 0; i < 6; ++i) CHECK(arena.capacity(0, i) == caps[i]);
  // 2. a second frame with equal or smaller requests: the same blocks, no allocation
  {
    Frame f(arena, 0);
    std::vector<Taken> live;
    const size_t again[6] = {288, 1000, 17, 787, 2000, 1};  // (288, 787: exactly the capacity)
    for (size_t b : again) take(f, live, b);
    check_live(live);
    CHECK(g_allocs == 6 && g_frees == 0);
  }
  // 3. growth of a later slot, and only where the capacity is below the request: earlier pointers stay valid, their
  // bytes intact
  {
    Frame f(arena, 0);
    std::vector<Taken> live;
    take(f, live, 200);
    take(f, live, 1125);
    CHECK(g_allocs == 6);
    take(f, live, 4609);  // one byte over slot 2's capacity
    CHECK(g_allocs == 7 && g_frees == 1 && g_last_alloc == 4609 + 4609 / 8);
    check_live(live);
    take(f, live, 100000);  // slot 3
    CHECK(g_allocs == 8 && g_frees == 2 && g_last_alloc == 100000 + 100000 / 8);
    check_live(live);
    CHECK(arena.capacity(0, 0) == 288 && arena.capacity(0, 1) == 1125 && arena.capacity(0, 4) == 2362);
  }
  // 4. growth followed by smaller requests: the grown blocks stay
  {
    Frame f(arena, 0);
    std::vector<Taken> live;
    for (size_t b : {8u, 8u, 8u, 8u}) take(f, live, b);
    check_live(live);
    CHECK(g_allocs == 8 && g_frees == 2 && arena.capacity(0, 3) == 112500);
  }
  // 5. another device has its own slot list
  {
    Frame f(arena, 1);
    std::vector<Taken> live;
    take(f, live, 5000);
    CHECK(g_allocs == 9 && g_frees == 2 && arena.num_slots(1) == 1 && arena.num_slots(0) == 6);
    CHECK(arena.capacity(1, 0) == 5625 && arena.capacity(0, 0) == 288);
  }
  {
    Frame f0(arena, 0);
    std::vector<Taken> live;
    take(f0, live, 288);
    CHECK(g_allocs == 9);
  }
  std::printf("ok %d checks, %d allocations, %d frees\n", g_checks, g_allocs, g_frees);
  return 0;
}
