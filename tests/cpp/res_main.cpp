// res_main.cpp — the ledger of whitebox_amd/csrc/wbx_res.h.  TEST INFRASTRUCTURE, a program of its own: the real header over a
// counting fake of the twelve HIP entry points it calls (malloc stands behind every handle, so the sanitizers see a leak, a
// double free and a use after free as well), no HIP library linked.  One line per case; exit status 1 on any imbalance.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -fsanitize=address,undefined -fno-sanitize-recover=all res_main.cpp
#include "../../whitebox_amd/csrc/wbx_res.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

namespace {
struct Ledger {
  int dev = 0, pinned = 0, events = 0, streams = 0;   // live handles
  int creates = 0, fail_at = 0;                       // creates so far / the one to fail (1-based, 0: none)
  int calls = 0;                                      // every fake entry point counts itself
  std::vector<std::string> log;                       // "free", "malloc", "record <ev> <stream>", "sync <ev>", ...
  hipError_t query = hipSuccess;
  int live() const { return dev + pinned + events + streams; }
} L;

void* make(int& n, hipError_t* e, const char* what) {
  L.calls++;
  if (++L.creates == L.fail_at) return *e = hipErrorOutOfMemory, nullptr;
  n++;
  L.log.push_back(what);
  return *e = hipSuccess, std::malloc(16);
}
hipError_t drop(int& n, void* p, const char* what) {
  L.calls++;
  n--;
  L.log.push_back(what);
  std::free(p);
  return hipSuccess;
}
std::string name(const char* verb, const void* a, const void* b = nullptr) {
  char t[96];
  std::snprintf(t, sizeof t, "%s %p %p", verb, a, b);
  return t;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t) { hipError_t e; *p = make(L.dev, &e, "malloc"); return e; }
hipError_t hipFree(void* p) { return drop(L.dev, p, "free"); }
hipError_t hipHostMalloc(void** p, size_t, unsigned) { hipError_t e; *p = make(L.pinned, &e, "host_malloc"); return e; }
hipError_t hipHostFree(void* p) { return drop(L.pinned, p, "host_free"); }
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) { hipError_t e; *ev = (hipEvent_t)make(L.events, &e, "event"); return e; }
hipError_t hipEventDestroy(hipEvent_t ev) { return drop(L.events, ev, "event_destroy"); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { hipError_t e; *s = (hipStream_t)make(L.streams, &e, "stream"); return e; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { hipError_t e; *s = (hipStream_t)make(L.streams, &e, "stream"); return e; }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(L.streams, s, "stream_destroy"); }
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s) { L.calls++; L.log.push_back(name("record", ev, s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t ev) { L.calls++; L.log.push_back(name("sync", ev)); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { L.calls++; return L.query; }
}

namespace {
using namespace wbx;
int failures = 0;

void begin() { L = Ledger{}; }
void expect(bool ok, const char* what) {
  if (!ok) std::printf("    FAILED: %s\n", what), failures++;
}
void end(const char* name) {
  expect(L.live() == 0, "the ledger is zero");
  std::printf("%s: dev %d pinned %d events %d streams %d after %d calls\n", name, L.dev, L.pinned, L.events, L.streams, L.calls);
}

// every holder: create then destroy, a double release, release of a holder never filled
void case_create_destroy() {
  begin();
  {
    DevBuf<float> d;
    PinnedBuf<int> p;
    Event ev;
    Stream s, sp;
    PinnedSlot<char> slot;
    expect(!d.p && !p.p && !ev.h && !s.h && !slot.buf.p && !slot.done.h && !slot.busy, "null by default");
    expect(d.ensure(10) == hipSuccess && d.p && d.cap == 10, "DevBuf::ensure");
    expect(p.ensure(7) == hipSuccess && p.p && p.cap == 7, "PinnedBuf::ensure");
    expect(ev.ensure(hipEventDisableTiming) == hipSuccess && ev.h, "Event::ensure");
    const hipEvent_t first = ev;
    expect(ev.ensure(hipEventDisableTiming) == hipSuccess && ev == first, "a second Event::ensure keeps the event");
    expect(s.create(hipStreamNonBlocking) == hipSuccess && s.h && s.owned, "Stream::create");
    expect(sp.create_with_priority(hipStreamNonBlocking, -1) == hipSuccess && sp.h && sp.owned, "Stream::create_with_priority");
    expect(slot.buf.ensure(3) == hipSuccess && slot.done.ensure(0) == hipSuccess, "PinnedSlot's members");
    expect(L.live() == 7, "seven live handles");
    d.release(), d.release();
    p.release(), p.release();
    ev.release(), ev.release();
    s.release(), s.release();
    expect(L.live() == 3 && !d.p && !d.cap && !p.p && !p.cap && !ev.h && !s.h, "a double release frees once and leaves null");
  }   // sp and slot go by their destructors
  end("create_destroy");
}

// growth: the old block is freed before the new one exists in the holder; no growth: no call
void case_growth() {
  begin();
  {
    DevBuf<double> d;
    PinnedBuf<double> p;
    expect(d.ensure(4) == hipSuccess && p.ensure(4) == hipSuccess, "first ensure");
    const int before = L.calls;
    expect(d.ensure(4) == hipSuccess && d.ensure(2) == hipSuccess && p.ensure(3) == hipSuccess && L.calls == before, "no call when it fits");
    L.log.clear();
    expect(d.ensure(9) == hipSuccess && d.cap == 9 && L.dev == 1, "DevBuf grew");
    expect(p.ensure(9) == hipSuccess && p.cap == 9 && L.pinned == 1, "PinnedBuf grew");
    expect(L.log == std::vector<std::string>{"free", "malloc", "host_free", "host_malloc"}, "freed first, then allocated");
  }
  end("growth");
}

template <class H, class Make>
void move_case(const char* what, Make make) {
  H a;
  make(a);
  const int live = L.live();
  H b(std::move(a));
  expect(L.live() == live, what);
  H c;
  make(c);
  c = std::move(b);   // frees what c held
  expect(L.live() == live, what);
  H& self = c;
  c = std::move(self);   // (self-assignment keeps it)
  expect(L.live() == live, what);
  expect(std::is_copy_constructible<H>::value == false && std::is_copy_assignable<H>::value == false, "copy is deleted");
}

// a move leaves the source null and frees once
void case_moves() {
  begin();
  {
    DevBuf<float> a;
    (void)a.ensure(5);
    DevBuf<float> b(std::move(a));
    expect(!a.p && !a.cap && b.p && b.cap == 5, "DevBuf: the source is null");
    PinnedBuf<float> pa;
    (void)pa.ensure(5);
    PinnedBuf<float> pb;
    pb = std::move(pa);
    expect(!pa.p && !pa.cap && pb.p && pb.cap == 5, "PinnedBuf: the source is null");
    Event ea;
    (void)ea.ensure(0);
    Event eb(std::move(ea));
    expect(!ea.h && eb.h, "Event: the source is null");
    Stream sa;
    (void)sa.create(0);
    Stream sb(std::move(sa));
    expect(!sa.h && !sa.owned && sb.h && sb.owned, "Stream: the source is null");
    PinnedSlot<int> la;
    (void)la.buf.ensure(2), (void)la.done.ensure(0), (void)la.mark(sb);
    PinnedSlot<int> lb(std::move(la));
    expect(!la.buf.p && !la.done.h && !la.busy && lb.buf.p && lb.done.h && lb.busy, "PinnedSlot: the source is empty");
    move_case<DevBuf<int>>("DevBuf moves", [](DevBuf<int>& h) { (void)h.ensure(3); });
    move_case<PinnedBuf<int>>("PinnedBuf moves", [](PinnedBuf<int>& h) { (void)h.ensure(3); });
    move_case<Event>("Event moves", [](Event& h) { (void)h.ensure(0); });
    move_case<Stream>("Stream moves", [](Stream& h) { (void)h.create(0); });
    move_case<PinnedSlot<int>>("PinnedSlot moves", [](PinnedSlot<int>& h) { (void)h.buf.ensure(3), (void)h.done.ensure(0); });
  }
  end("moves");
}

// std::swap of two events (drain_events swaps timing events) keeps both and frees both
void case_swap() {
  begin();
  {
    Event a, b, none;
    (void)a.ensure(0), (void)b.ensure(0);
    const hipEvent_t ha = a, hb = b;
    std::swap(a, b);
    expect(a == hb && b == ha && L.events == 2, "swapped, none freed");
    std::swap(a, none);
    expect(!a.h && none == hb && L.events == 2, "swapped with an empty one");
  }
  end("swap");
}

// an adopted stream is the caller's: never destroyed, by release, by the destructor or by being replaced
void case_adopt() {
  begin();
  hipError_t e;
  const hipStream_t callers = (hipStream_t)make(L.streams, &e, "stream");
  {
    Stream s;
    s.adopt(callers);
    expect(s == callers && !s.owned, "adopted");
    Stream t(std::move(s));
    expect(t == callers && !t.owned && !s.h, "moved as adopted");
    t.release();
    expect(L.streams == 1 && !t.h, "release leaves it alone");
    t.adopt(callers);
    expect(t.create(0) == hipSuccess && t.owned && L.streams == 2, "a stream of its own takes the adopted one's place");
    t.adopt(callers);
    expect(L.streams == 1 && !t.owned, "... and is destroyed when one is adopted again");
  }
  expect(L.streams == 1, "the destructor leaves it alone");
  (void)drop(L.streams, callers, "stream_destroy");
  end("adopt");
}

// the n-th create fails: the holder is null, the error comes back, nothing is left after the scope
void case_failures() {
  begin();
  {
    L.fail_at = 1;
    DevBuf<int> d;
    expect(d.ensure(3) == hipErrorOutOfMemory && !d.p && !d.cap, "DevBuf: first create fails");
    expect(d.ensure(3) == hipSuccess, "DevBuf: and then works");
    L.fail_at = L.creates + 1;
    expect(d.ensure(6) == hipErrorOutOfMemory && !d.p && !d.cap && L.dev == 0, "DevBuf: growth fails, the old block is gone");
    L.fail_at = L.creates + 1;
    PinnedBuf<int> p;
    expect(p.ensure(3) == hipErrorOutOfMemory && !p.p && !p.cap, "PinnedBuf: create fails");
    L.fail_at = L.creates + 1;
    Event ev;
    expect(ev.ensure(0) == hipErrorOutOfMemory && !ev.h, "Event: create fails");
    L.fail_at = L.creates + 1;
    Stream s;
    expect(s.create(0) == hipErrorOutOfMemory && !s.h && !s.owned, "Stream: create fails");
    L.fail_at = L.creates + 1;
    expect(s.create_with_priority(0, 0) == hipErrorOutOfMemory && !s.h && !s.owned, "Stream: create_with_priority fails");
  }
  end("failures");
}

// three slots grown together the way ensure_pinned_tables grows the patch and gain tables (buffer, buffer, event, event per
// slot; the first failure returns), then grown again — with every create of that sequence failing in turn
hipError_t grow_tables(PinnedSlot<int> (&a)[3], PinnedSlot<float> (&b)[3], size_t cap) {
  for (int i = 0; i < 3; i++) {
    hipError_t e = a[i].buf.ensure(cap);
    if (e == hipSuccess) e = b[i].buf.ensure(cap * 2);
    a[i].forget(), b[i].forget();
    if (e == hipSuccess) e = a[i].done.ensure(0);
    if (e == hipSuccess) e = b[i].done.ensure(0);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
void case_slot_array_failures() {
  int total = 0;
  {
    begin();
    PinnedSlot<int> a[3];
    PinnedSlot<float> b[3];
    expect(grow_tables(a, b, 8) == hipSuccess && grow_tables(a, b, 16) == hipSuccess, "no failure: both rounds work");
    total = L.creates;
    expect(total == 12 + 6 && L.pinned == 6 && L.events == 6, "12 creates, then 6 to grow");
  }
  expect(L.live() == 0, "the ledger is zero");
  for (int n = 1; n <= total; n++) {
    begin();
    L.fail_at = n;
    {
      PinnedSlot<int> a[3];
      PinnedSlot<float> b[3];
      hipError_t e = grow_tables(a, b, 8);
      if (e == hipSuccess) e = grow_tables(a, b, 16);
      expect(e == hipErrorOutOfMemory, "the error is returned");
      int nulls = 0;
      for (int i = 0; i < 3; i++) {
        nulls += !a[i].buf.p + !b[i].buf.p + !a[i].done.h + !b[i].done.h;
        expect(!a[i].buf.p == !a[i].buf.cap && !b[i].buf.p == !b[i].buf.cap, "null and empty together");
      }
      expect(nulls >= 1 && 12 - nulls == L.live(), "the holder whose create failed is null, the live ones are the others");
    }
    expect(L.live() == 0, "the ledger is zero after the scope");
  }
  begin();
  std::printf("slot_array_failures: %d creates, each failed in turn\n", total);
}

// the slot's verbs
void case_slot_verbs() {
  begin();
  hipError_t e;
  const hipStream_t s = (hipStream_t)make(L.streams, &e, "stream");
  {
    PinnedSlot<int> slot;
    (void)slot.done.ensure(hipEventDisableTiming);
    int before = L.calls;
    expect(slot.wait() == hipSuccess && L.calls == before, "wait on a fresh slot makes no call");
    expect(slot.idle() && L.calls == before, "a fresh slot is idle, no call");
    L.log.clear();
    expect(slot.mark(s) == hipSuccess && slot.busy, "mark");
    expect(L.log == std::vector<std::string>{name("record", slot.done.h, s)}, "mark records the slot's event on that stream");
    L.log.clear();
    expect(slot.wait() == hipSuccess, "wait");
    expect(L.log == std::vector<std::string>{name("sync", slot.done.h)}, "the next wait synchronises exactly that event");
    L.query = hipErrorNotReady;
    expect(!slot.idle(), "idle follows the query: not ready");
    L.query = hipSuccess;
    expect(slot.idle(), "idle follows the query: ready");
    slot.forget();
    before = L.calls;
    expect(!slot.busy && slot.wait() == hipSuccess && L.calls == before, "after forget the wait is a no-op");
    L.query = hipErrorNotReady;
    expect(slot.idle() && L.calls == before, "... and the slot idle without a query");
  }
  (void)drop(L.streams, s, "stream_destroy");
  end("slot_verbs");
}
}  // namespace

int main() {
  case_create_destroy();
  case_growth();
  case_moves();
  case_swap();
  case_adopt();
  case_failures();
  case_slot_array_failures();
  case_slot_verbs();
  if (failures) std::printf("res_main FAILED %d checks\n", failures);
  else std::printf("res_main ok\n");
  return failures ? 1 : 0;
}
