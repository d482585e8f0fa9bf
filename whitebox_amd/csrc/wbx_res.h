// wbx_res.h — the holders of what the host side takes from the HIP runtime: device arrays, pinned host blocks, events and
// streams.  The one place that frees them.  Plain host C++ (no kernels, no environment, nothing of wbx_ctx.h).
//
// Every holder is move-only, null by default and releases in its destructor, ignoring the error.  A destructor never
// waits and never chooses the device: whoever drops a holder the device may still use waits first, where the code says so.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace wbx {

template <class T>
struct DevBuf {             // grow-only device array (growing frees the old block first and keeps no contents)
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

template <class T>
struct PinnedBuf {          // the same over pinned host memory, which the device reads and writes in place
  T* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~PinnedBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct Event {              // reads as its handle: hipEventRecord(ev, s)
  hipEvent_t h = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      release();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~Event() { release(); }
  hipError_t ensure(unsigned flags) {   // made at first use; the flags of that call are the event's
    if (h) return hipSuccess;
    const hipError_t e = hipEventCreateWithFlags(&h, flags);
    if (e != hipSuccess) h = nullptr;
    return e;
  }
  void release() {
    if (h) (void)hipEventDestroy(h);
    h = nullptr;
  }
  operator hipEvent_t() const { return h; }
};

struct Stream {             // reads as its handle; an adopted stream is the caller's and is never destroyed
  hipStream_t h = nullptr;
  bool owned = false;
  Stream() = default;
  Stream(Stream&& o) noexcept : h(std::exchange(o.h, nullptr)), owned(std::exchange(o.owned, false)) {}
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) {
      release();
      h = std::exchange(o.h, nullptr);
      owned = std::exchange(o.owned, false);
    }
    return *this;
  }
  ~Stream() { release(); }
  hipError_t create(unsigned flags) {
    release();
    return made(hipStreamCreateWithFlags(&h, flags));
  }
  hipError_t create_with_priority(unsigned flags, int priority) {
    release();
    return made(hipStreamCreateWithPriority(&h, flags, priority));
  }
  void adopt(hipStream_t s) {
    release();
    h = s;
  }
  void release() {
    if (h && owned) (void)hipStreamDestroy(h);
    h = nullptr;
    owned = false;
  }
  operator hipStream_t() const { return h; }

 private:
  hipError_t made(hipError_t e) {
    if (e == hipSuccess) owned = true;
    else h = nullptr;
    return e;
  }
};

// A pinned buffer the device reads (or a copy fills) in place, the event of its last user and whether there is one: the
// host waits before it refills the buffer, marks it behind the work that uses it, and forgets a user it knows to be over.
template <class T>
struct PinnedSlot {
  PinnedBuf<T> buf;
  Event done;               // (made by its owner, with the flags that owner needs: done.ensure)
  bool busy = false;
  PinnedSlot() = default;
  PinnedSlot(PinnedSlot&& o) noexcept : buf(std::move(o.buf)), done(std::move(o.done)), busy(std::exchange(o.busy, false)) {}
  PinnedSlot& operator=(PinnedSlot&& o) noexcept {
    if (this != &o) {
      buf = std::move(o.buf);
      done = std::move(o.done);
      busy = std::exchange(o.busy, false);
    }
    return *this;
  }
  hipError_t wait() { return busy ? hipEventSynchronize(done) : hipSuccess; }
  bool idle() const { return !busy || hipEventQuery(done) == hipSuccess; }
  hipError_t mark(hipStream_t s) {
    const hipError_t e = hipEventRecord(done, s);
    if (e == hipSuccess) busy = true;
    return e;
  }
  void forget() { busy = false; }
};

}  // namespace wbx
