// pool_sim.cpp — wbx_pool.h (the clip pool's extent policy, the product's own source) on the CPU behind a C interface:
// a slab list, a table of the extents handed out and a "driver" that hands out no memory at all and can be told to fail.
// TEST INFRASTRUCTURE: tests/pool_sim.py builds and drives it, tests/test_pool_model.py compares every placement with
// tests/pool_model.py; tests/cpp/pool_main.cpp includes this file for its stand-alone sanitizer run.
#include <cstdint>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_pool.h"

namespace {

struct Extent {
  int slab = -1;   // index in the slab list, -1: an allocation of its own
  size_t off = 0, len = 0;
  bool live = false;
};

struct Sim {
  wbx::ClipSlabs slabs;
  std::vector<Extent> extents;
  uint64_t limit = 0, own_reserved = 0;
  bool driver_fails = false;
  uint64_t driver_calls = 0;
};

char g_memory;   // every slab's "memory": never read or written, only tested for nullptr

char* driver(void* user, size_t) {
  Sim* s = (Sim*)user;
  s->driver_calls++;
  return s->driver_fails ? nullptr : &g_memory;
}

}  // namespace

extern "C" {

void* psim_create() { return new Sim(); }
void psim_destroy(void* h) { delete (Sim*)h; }
void psim_set_limit(void* h, uint64_t limit) { ((Sim*)h)->limit = limit; }
void psim_set_driver_fails(void* h, int fails) { ((Sim*)h)->driver_fails = fails != 0; }

// wbx::pool_extent: the granules of a clip of `bytes` that is the (placed + 1)-th of its context
void psim_extent(uint64_t bytes, uint32_t placed, int jitter, uint64_t* body, uint64_t* gap) {
  const wbx::PoolExtent e = wbx::pool_extent((size_t)bytes, placed, jitter != 0);
  *body = e.body;
  *gap = e.gap;
}

// -> wbx::PoolWhere; for POOL_IN_SLAB and POOL_OWN *id names the extent for psim_give
int psim_take(void* h, uint64_t need, uint64_t own_bytes, int use_slabs, uint32_t* id, int32_t* slab, uint64_t* off) {
  Sim* s = (Sim*)h;
  const wbx::PoolTake t = wbx::pool_take(s->slabs, (size_t)need, (size_t)own_bytes, s->limit, s->own_reserved, use_slabs != 0, driver, s);
  *slab = -1;
  *off = 0;
  *id = ~0u;
  Extent e;
  e.live = true;
  if (t.where == wbx::POOL_IN_SLAB) {
    for (size_t i = 0; i < s->slabs.size(); i++)
      if (s->slabs[i].get() == t.slab) e.slab = (int)i;
    e.off = t.off;
    e.len = (size_t)need;
    *slab = e.slab;
    *off = e.off;
  } else if (t.where == wbx::POOL_OWN) {
    e.len = (size_t)own_bytes;
    s->own_reserved += own_bytes;
  } else {
    return (int)t.where;
  }
  *id = (uint32_t)s->extents.size();
  s->extents.push_back(e);
  return (int)t.where;
}

int psim_give(void* h, uint32_t id) {
  Sim* s = (Sim*)h;
  if (id >= s->extents.size() || !s->extents[id].live) return -1;
  Extent& e = s->extents[id];
  if (e.slab >= 0)
    wbx::pool_give(*s->slabs[(size_t)e.slab], e.off, e.len);
  else
    s->own_reserved -= e.len;
  e.live = false;
  return 0;
}

// wbx_clip_pool_stats: the slabs' share from the header, the clips with an allocation of their own added as the library does
void psim_stats(void* h, uint32_t* n_slabs, uint64_t* bytes_reserved, uint64_t* bytes_live, uint64_t* driver_calls) {
  Sim* s = (Sim*)h;
  wbx::pool_slab_stats(s->slabs, n_slabs, bytes_reserved, bytes_live);
  *bytes_reserved += s->own_reserved;
  *bytes_live += s->own_reserved;
  *driver_calls = s->driver_calls;
}

// one slab's books: info = {size, used, live, live_bytes}; holes as (offset, bytes) pairs, at most cap of them written;
// -> the number of holes, -1: no such slab
int psim_dump(void* h, uint32_t slab, uint64_t info[4], uint64_t* holes, uint32_t cap) {
  Sim* s = (Sim*)h;
  if (slab >= s->slabs.size()) return -1;
  const wbx::ClipSlab& sl = *s->slabs[slab];
  info[0] = sl.size;
  info[1] = sl.used;
  info[2] = sl.live;
  info[3] = sl.live_bytes;
  for (size_t i = 0; i < sl.holes.size() && i < cap; i++) {
    holes[2 * i] = sl.holes[i].first;
    holes[2 * i + 1] = sl.holes[i].second;
  }
  return (int)sl.holes.size();
}

}  // extern "C"
