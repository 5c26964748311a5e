// lsm2d_capi_own.h -- who owns what on the host side of the C ABI: move-only owners of a device buffer, a pinned host buffer, an event and a stream.
// A resource is released because its owner goes away (or is reset), never by a line somebody has to remember.  Host only: no kernels, nothing of lsm2d.h,
// no exceptions.  Every acquisition returns the runtime's hipError_t, so the call sites keep their HIPCHK.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <utility>

namespace lsm2d {

// Handles alive in this process: counted up where an owner acquires, down where it releases, and nowhere else ("live_handles", lsm2d_get_option).  Process-wide
// and not a context's, because a set may outlive its context.
inline std::atomic<long long> g_live_handles{0};
inline long long live_handles() { return g_live_handles.load(std::memory_order_relaxed); }

// The part the four owners share: one handle, released by Release unless it is only borrowed.
template <class H, hipError_t (*Release)(H)> class Owner {
 public:
  Owner() = default;
  Owner(const Owner&) = delete; Owner& operator=(const Owner&) = delete;
  Owner(Owner&& o) noexcept : h_(o.h_), owned_(o.owned_) { o.h_ = H(); o.owned_ = false; }
  Owner& operator=(Owner&& o) noexcept { if (this != &o) { reset(); h_ = o.h_; owned_ = o.owned_; o.h_ = H(); o.owned_ = false; } return *this; }
  ~Owner() { reset(); }
  void reset() {
    if (h_ && owned_) { (void) Release(h_); g_live_handles.fetch_sub(1, std::memory_order_relaxed); }
    h_ = H(); owned_ = false;
  }
  explicit operator bool() const { return h_ != H(); }

 protected:
  // What an acquiring call ends with: on success the fresh handle is owned, on failure the owner stays empty.  (The runtime call that fills `h` comes first, in a
  // statement of its own: a call's arguments are evaluated in no fixed order.)
  hipError_t acquired(hipError_t e, H h) {
    if (e == hipSuccess) { h_ = h; owned_ = true; g_live_handles.fetch_add(1, std::memory_order_relaxed); }
    return e;
  }
  H h_ = H(); bool owned_ = false;      // (borrowed: held, not owned)
};

// hipMalloc / hipFree.  T is what the buffer holds; void: a block that its users carve up, and only such a block converts to any pointer type under a cast.
template <class T> struct OnlyVoid {}; template <> struct OnlyVoid<void> { typedef int type; };
template <class T = void> class DevBuf : public Owner<void*, hipFree> {
 public:
  hipError_t alloc(size_t bytes) { reset(); void* p = nullptr; const hipError_t e = hipMalloc(&p, bytes); return acquired(e, p); }
  T* get() const { return static_cast<T*>(h_); }
  operator T*() const { return get(); }
  template <class U, class V = T, class = typename OnlyVoid<V>::type> explicit operator U*() const { return (U*) h_; }
};

// hipHostMalloc with the caller's flags / hipHostFree.  Mapped memory's device-side address is looked up once (dev()); kernels with small outputs write there.
class PinnedBuf : public Owner<void*, hipHostFree> {
 public:
  hipError_t alloc(size_t bytes, unsigned flags) {
    reset(); void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, flags);
    e = acquired(e, p);
    if (e == hipSuccess && (flags & hipHostMallocMapped)) { e = hipHostGetDevicePointer(&dev_, h_, 0); if (e != hipSuccess) reset(); }
    return e;
  }
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : Owner(std::move(o)), dev_(o.dev_) { o.dev_ = nullptr; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { Owner::operator=(std::move(o)); dev_ = o.dev_; o.dev_ = nullptr; } return *this; }
  void reset() { Owner::reset(); dev_ = nullptr; }
  void* get() const { return h_; }
  void* dev() const { return dev_; }
  operator void*() const { return h_; }
  template <class U> explicit operator U*() const { return (U*) h_; }

 private:
  void* dev_ = nullptr;
};

class Event : public Owner<hipEvent_t, hipEventDestroy> {
 public:
  hipError_t create(unsigned flags = hipEventDefault) { reset(); hipEvent_t ev = nullptr; const hipError_t e = hipEventCreateWithFlags(&ev, flags); return acquired(e, ev); }
  hipEvent_t get() const { return h_; }
  operator hipEvent_t() const { return h_; }
};

class Stream : public Owner<hipStream_t, hipStreamDestroy> {
 public:
  hipError_t create(unsigned flags) { reset(); hipStream_t s = nullptr; const hipError_t e = hipStreamCreateWithFlags(&s, flags); return acquired(e, s); }
  hipError_t create(unsigned flags, int priority) { reset(); hipStream_t s = nullptr; const hipError_t e = hipStreamCreateWithPriority(&s, flags, priority); return acquired(e, s); }
  void borrow(hipStream_t s) { reset(); h_ = s; }      // the caller's stream: used, never destroyed, not counted
  hipStream_t get() const { return h_; }
  operator hipStream_t() const { return h_; }
};

// A buffer that grows on demand, with the bytes it holds.  ensure() is the free / allocate / remember part of every such site; the site keeps its headroom
// rule (`cap`), its refusals and flags, and -- `before_free`, called only when an old block is about to go -- its wait for whoever may still use that block.
template <class Buf> struct Grown : Buf {
  size_t bytes = 0;
  Grown() = default;
  Grown(Grown&&) = delete;
  void reset() { Buf::reset(); bytes = 0; }
  template <class BeforeFree, class... Flags> hipError_t ensure(size_t need, size_t cap, BeforeFree before_free, Flags... flags) {
    if (need <= bytes) return hipSuccess;
    if (*this) { const hipError_t e = before_free(); if (e != hipSuccess) return e; reset(); }
    const hipError_t e = Buf::alloc(cap, flags...);
    if (e == hipSuccess) bytes = cap;
    return e;
  }
};

}  // namespace lsm2d
