// capi_own_driver.cpp -- the owners of srrg2_laser_slam_2d_amd/csrc/lsm2d_capi_own.h on the host alone: this file defines the handful of HIP functions the header
// calls, backed by malloc / free with a count of their own, and links against no HIP library.  Built with -fsanitize=address,undefined by
// tests/test_capi_own_cpu.py: a leak, a double release or a use after release ends the run with a sanitizer report; a failed CHECK ends it with status 1.
// At every step the header's live count must equal the stand-ins' count, and both must be 0 at the end.
#include "lsm2d_capi_own.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

namespace {
std::set<void*> g_live;            // what the stand-ins handed out and have not taken back
long long g_acquisitions = 0;      // acquisitions asked for so far
long long g_fail_at = 0;           // > 0: the acquisition with this number fails with hipErrorOutOfMemory
int g_device_lookups = 0;          // hipHostGetDevicePointer calls
constexpr long kDeviceAlias = 0x1000;      // the "device-side address" of a mapped block: its host address plus this

hipError_t acquire(void** out, size_t bytes) {
  *out = nullptr;
  if (++g_acquisitions == g_fail_at) return hipErrorOutOfMemory;
  void* p = malloc(bytes ? bytes : 1);
  if (!p) return hipErrorOutOfMemory;
  g_live.insert(p); *out = p;
  return hipSuccess;
}
hipError_t give_back(void* p) {
  if (!g_live.erase(p)) { fprintf(stderr, "released what was not live: %p\n", p); exit(2); }
  free(p);
  return hipSuccess;
}
void fail_next() { g_fail_at = g_acquisitions + 1; }
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return acquire(p, bytes); }
hipError_t hipFree(void* p) { return give_back(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return acquire(p, bytes); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) { ++g_device_lookups; *dev = (char*) host + kDeviceAlias; return hipSuccess; }
hipError_t hipHostFree(void* p) { return give_back(p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return acquire((void**) e, 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return give_back(e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return acquire((void**) s, 1); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return acquire((void**) s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return give_back(s); }
hipError_t hipGetLastError(void) { return hipSuccess; }
}

using namespace lsm2d;

// REQUIRE: the condition alone; CHECK: ... and the two counts agree
#define REQUIRE(cond)                                                                                     \
  do {                                                                                                    \
    if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); }   \
  } while (0)
#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    REQUIRE(cond);                                                                                        \
    if (live_handles() != (long long) g_live.size()) {                                                    \
      fprintf(stderr, "%s:%d: the header counts %lld live handles, the stand-ins %zu\n", __FILE__, __LINE__, live_handles(), g_live.size());      \
      exit(1);                                                                                            \
    }                                                                                                     \
  } while (0)
#define LIVE(n) CHECK(live_handles() == (n))

// what GridCache / KdCache are to a set: a struct with plain fields, an owner and views into its block
struct Cache {
  float key = 0.0f;
  DevBuf<> block;
  int* view = nullptr;
};

static Cache make_cache(float key) {
  Cache c; c.key = key;
  REQUIRE(c.block.alloc(64) == hipSuccess);
  c.view = (int*) c.block;
  c.view[0] = (int) key;
  return c;
}

static void moves() {
  DevBuf<int> a;
  CHECK(!a && a.get() == nullptr);
  CHECK(a.alloc(16 * sizeof(int)) == hipSuccess && a);
  LIVE(1);
  int* const p = a;
  a.get()[3] = 7;
  DevBuf<int> b(std::move(a));                      // move construction
  CHECK(!a && b.get() == p && b[3] == 7);
  LIVE(1);
  DevBuf<int> c;
  CHECK(c.alloc(4) == hipSuccess);
  LIVE(2);
  c = std::move(b);                                 // move assignment releases what the target held
  CHECK(!b && c.get() == p);
  LIVE(1);
  DevBuf<int>& self = c;
  c = std::move(self);                              // self-move: nothing happens
  CHECK(c.get() == p && c[3] == 7);
  LIVE(1);
  c.reset(); c.reset();                             // reset twice
  CHECK(!c);
  LIVE(0);
  CHECK(c.alloc(8) == hipSuccess && c.alloc(8) == hipSuccess);      // allocating again replaces
  LIVE(1);
  {
    DevBuf<int> d(std::move(c));
    DevBuf<int> gone(std::move(d));                 // d: a moved-from owner destroyed at the brace
    LIVE(1);
  }
  LIVE(0);
  fail_next();
  CHECK(c.alloc(8) == hipErrorOutOfMemory && !c);   // a failed acquisition leaves the owner empty
  LIVE(0);
}

static void events_and_streams() {
  Event e, f;
  CHECK(e.create() == hipSuccess && f.create(hipEventDisableTiming) == hipSuccess && e && f);
  LIVE(2);
  hipEvent_t raw = e;
  Event g(std::move(e));
  CHECK(!e && g.get() == raw);
  f = std::move(g);
  CHECK(f.get() == raw);
  LIVE(1);
  fail_next();
  CHECK(e.create() == hipErrorOutOfMemory && !e);
  Stream own, prio;
  CHECK(own.create(hipStreamNonBlocking) == hipSuccess && prio.create(hipStreamNonBlocking, -1) == hipSuccess);
  LIVE(3);
  // the caller's stream: used, never destroyed, never counted (so the comparison of the two counts rests until it is given back: REQUIRE, not CHECK)
  void* callers = nullptr;
  REQUIRE(acquire(&callers, 1) == hipSuccess);
  const size_t with_callers = g_live.size();
  {
    Stream borrowed;
    borrowed.borrow((hipStream_t) callers);
    REQUIRE(borrowed && borrowed.get() == (hipStream_t) callers && g_live.size() == with_callers && live_handles() == 3);
    Stream moved(std::move(borrowed));
    moved.reset();
    Stream again; again.borrow((hipStream_t) callers);
    prio = std::move(again);                        // the owned stream under it goes, the borrowed one stays the caller's
    REQUIRE(g_live.size() == with_callers - 1 && live_handles() == 2 && g_live.count(callers) == 1);
  }
  prio.reset();
  REQUIRE(g_live.count(callers) == 1);      // the caller's stream was not destroyed
  (void) give_back(callers);
  LIVE(2);
}

static void pinned() {
  PinnedBuf plain, mapped;
  g_device_lookups = 0;
  CHECK(plain.alloc(256, hipHostMallocDefault) == hipSuccess && plain.dev() == nullptr && g_device_lookups == 0);
  CHECK(mapped.alloc(256, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess && g_device_lookups == 1);
  CHECK(mapped.dev() == (char*) mapped.get() + kDeviceAlias);
  CHECK(mapped.dev() == (char*) mapped.get() + kDeviceAlias && g_device_lookups == 1);      // looked up once
  LIVE(2);
  void* const dev = mapped.dev();
  PinnedBuf m2(std::move(mapped));
  CHECK(!mapped && mapped.dev() == nullptr && m2.dev() == dev);
  plain = std::move(m2);
  CHECK(plain.dev() == dev);
  LIVE(1);
  plain.reset();
  CHECK(plain.dev() == nullptr);
  LIVE(0);
}

static void caches_in_a_vector() {
  std::vector<Cache> v;
  for (int i = 0; i < 9; ++i) v.push_back(make_cache((float) i));      // reallocates several times: every element moves, none is released
  LIVE(9);
  for (int i = 0; i < 9; ++i) CHECK(v[(size_t) i].view == (int*) v[(size_t) i].block && v[(size_t) i].view[0] == i);
  v.erase(v.begin() + 2);
  LIVE(8);
  CHECK(v[2].view[0] == 3);
  // a block moves out of an element and back into a new one: the KD-tree's recycled allocation
  DevBuf<> kept = std::move(v[0].block);
  v.clear();
  LIVE(1);
  Cache c; c.block = std::move(kept); c.view = (int*) c.block;
  v.push_back(std::move(c));
  CHECK(v[0].view[0] == 0);
  LIVE(1);
  v.clear();
  LIVE(0);
}

static void grow() {
  int waits = 0;
  auto wait = [&waits] { ++waits; return hipSuccess; };
  Grown<DevBuf<>> g;
  CHECK(g.ensure(100, 100 + 50 + 4096, wait) == hipSuccess && g && g.bytes == 4246 && waits == 0);      // nothing to wait for: there was no old block
  LIVE(1);
  void* const first = g.get();
  CHECK(g.ensure(4246, 1 << 20, wait) == hipSuccess && g.get() == first && g.bytes == 4246 && waits == 0);      // a smaller (or equal) request keeps the buffer
  CHECK(g.ensure(4247, 8000, wait) == hipSuccess && g.bytes == 8000 && waits == 1);                             // a larger one replaces it, after the wait
  LIVE(1);
  fail_next();
  CHECK(g.ensure(9000, 9000, wait) == hipErrorOutOfMemory && !g && g.bytes == 0 && waits == 2);                 // a failed allocation: pointer null, size 0
  LIVE(0);
  CHECK(g.ensure(1, 1, wait) == hipSuccess && g.bytes == 1 && waits == 2);
  // a wait that fails keeps the old block
  void* const kept = g.get();
  CHECK(g.ensure(2, 2, [] { return hipErrorUnknown; }) == hipErrorUnknown && g.get() == kept && g.bytes == 1);
  LIVE(1);
  Grown<PinnedBuf> h;
  CHECK(h.ensure(10, 26, wait, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess && h.bytes == 26 && h.dev() == (char*) h.get() + kDeviceAlias);
  LIVE(2);
  h.reset();
  CHECK(h.bytes == 0 && h.dev() == nullptr);
  LIVE(1);
}

int main() {
  moves();
  LIVE(0);
  events_and_streams();
  LIVE(0);
  pinned();
  LIVE(0);
  caches_in_a_vector();
  LIVE(0);
  grow();
  LIVE(0);
  if (!g_live.empty() || live_handles() != 0) { fprintf(stderr, "%zu handles left, the header counts %lld\n", g_live.size(), live_handles()); return 1; }
  printf("owners ok: %lld acquisitions, none left\n", g_acquisitions);
  return 0;
}
