// wbx_pool.h — where a clip's audio goes inside the clip pool: the slabs, the extents handed out of them and given back,
// the gap in front of a clip.  The ONLY home of that policy.  Plain C++ (no HIP, no wbx_ctx, no lock): clip_build,
// clip_release and wbx_clip_pool_stats (wbx_runtime.hip) call it with slab_mu held and hipMalloc behind the callback;
// tests/cpp/pool_sim.cpp and tests/cpp/pool_main.cpp compile it with g++ alone and a callback that hands out no memory
// at all, and tests/pool_model.py states the same policy a second time, over one bitmap of granules per slab.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <new>
#include <utility>
#include <vector>

namespace wbx {

constexpr size_t kPoolSlab = (size_t)1 << 30, kPoolGranule = (size_t)64 << 10;   // (8-GiB slabs, 2-MiB granules: no difference)
constexpr size_t kPoolSlabbed = kPoolSlab / 4;   // the largest extent a slab hands out; larger clips get an allocation of their own

// Clip audio lives in slabs of 1 GiB carved up in order (64-KiB granules): a session of thousands of clips is a few
// dozen large allocations, which the driver backs with large contiguous fragments (measured: the mix kernel's launch time
// is bimodal from process to process with one allocation per clip, 3-5 % apart, and stays at the fast end with slabs,
// tools/ab_arena.sh).  A slab's space is reused when the last clip in it has been freed; slabs go back to the
// driver with the context.  Clips above 256 MiB get an allocation of their own.
struct ClipSlab {
  char* mem = nullptr;
  size_t size = 0, used = 0;   // [0, used): handed out in order (bump); [used, size): untouched
  uint32_t live = 0;           // clips inside
  size_t live_bytes = 0;
  // extents below `used` that released clips gave back, sorted by offset, neighbours merged: first-fit for the next clip
  // that fits (replacing a clip again and again, or add / delete cycles beside a long-lived clip, stay inside the slab)
  std::vector<std::pair<size_t, size_t>> holes;   // (offset, bytes)
};
using ClipSlabs = std::vector<std::unique_ptr<ClipSlab>>;

// A pseudo-random gap of 0..15 granules in front of every clip (at most an eighth of the clip): a session of equally
// long clips has one clip-to-clip stride, and some strides alias in the HBM address hash — the workgroups in flight
// read the same offset of many clips at once (c4 with 9.06-MiB clips: 0.82 instead of 0.73 ms per launch;
// tools/ab_arena.sh).  `placed`: clips placed before this one (wbx_ctx::slab_seq); `bytes`: the clip's channel rows.
struct PoolExtent {
  size_t body = 0, gap = 0;   // the rows rounded up to granules; the granules in front of them.  The extent is gap + body.
};
inline PoolExtent pool_extent(size_t bytes, uint32_t placed, bool jitter) {
  PoolExtent e;
  e.body = (bytes + kPoolGranule - 1) / kPoolGranule * kPoolGranule;
  const uint32_t span = (uint32_t)std::min<size_t>(16, e.body / kPoolGranule / 8 + 1);
  e.gap = jitter ? (size_t)((((placed + 1u) * 2654435761u) >> 8) % span) * kPoolGranule : 0;
  return e;
}

// the driver's side of the pool: `bytes` of device memory or nullptr (a device too full is no error: see pool_take)
typedef char* (*PoolAlloc)(void* user, size_t bytes);

enum PoolWhere {
  POOL_IN_SLAB = 0,   // slab / off: booked
  POOL_OWN = 1,       // the caller allocates own_bytes for this clip alone (nothing booked here)
  POOL_LIMIT = 2,     // refused: wbx_clip_pool_limit
  POOL_NOMEM = 3,     // refused: the host is out of memory
};
struct PoolTake {
  PoolWhere where = POOL_NOMEM;
  ClipSlab* slab = nullptr;
  size_t off = 0;
};

inline uint64_t pool_slab_bytes(const ClipSlabs& slabs) {
  uint64_t r = 0;
  for (auto& sl : slabs) r += sl->size;
  return r;
}

// An extent of `need` bytes (whole granules, the gap included): the newest slab first — its lowest hole that fits, else
// its tail — then the older ones; else a new slab (64 MiB, 256 MiB, 1 GiB, 1 GiB ...: small sessions stay small).
// `limit` (0: none) bounds slabs + own_reserved, the bytes of the clips that have an allocation of their own: the usual
// slab if it fits, else one just large enough, else none.  A clip above kPoolSlabbed, any clip with use_slabs off (the
// pool model's other arm: the library passes true) and a clip that needs a new slab the driver cannot give get an allocation
// of own_bytes.
inline PoolTake pool_take(ClipSlabs& slabs, size_t need, size_t own_bytes, uint64_t limit, uint64_t own_reserved, bool use_slabs,
                          PoolAlloc alloc, void* user) {
  PoolTake t;
  if (use_slabs && need <= kPoolSlabbed) {
    ClipSlab* sl = nullptr;
    size_t at = 0;
    bool in_hole = false;
    for (auto it = slabs.rbegin(); it != slabs.rend() && !sl; ++it) {
      ClipSlab& cand = **it;
      for (auto h = cand.holes.begin(); h != cand.holes.end(); ++h)
        if (h->second >= need) {
          sl = &cand;
          at = h->first;
          in_hole = true;
          if (h->second == need) {
            cand.holes.erase(h);
          } else {
            h->first += need;
            h->second -= need;
          }
          break;   // (h may be gone)
        }
      if (!sl && cand.size - cand.used >= need) sl = &cand;
    }
    if (!sl) {
      std::unique_ptr<ClipSlab> fresh(new (std::nothrow) ClipSlab());
      if (!fresh) return t;
      const size_t grown = slabs.size() >= 2 ? kPoolSlab : ((size_t)64 << 20) << (2 * slabs.size());
      size_t sz = std::max(grown, need);
      if (limit) {
        const uint64_t have = pool_slab_bytes(slabs) + own_reserved;
        if (have + sz > limit) sz = need;
        if (have + sz > limit) {
          t.where = POOL_LIMIT;
          return t;
        }
      }
      if ((fresh->mem = alloc(user, sz)) != nullptr) {
        fresh->size = sz;
        slabs.push_back(std::move(fresh));
        sl = slabs.back().get();
      }
    }
    if (sl) {
      if (!in_hole) {
        at = sl->used;
        sl->used += need;
      }
      sl->live++;
      sl->live_bytes += need;
      t.where = POOL_IN_SLAB;
      t.slab = sl;
      t.off = at;
      return t;
    }
  }
  t.where = limit && pool_slab_bytes(slabs) + own_reserved + own_bytes > limit ? POOL_LIMIT : POOL_OWN;
  return t;
}

// the extent [off, off + len) of `sl` back: the last clip of a slab empties it; the newest extent steps the bump pointer
// back (over a hole that ends there, too); any other becomes a hole, merged with its neighbours
inline void pool_give(ClipSlab& sl, size_t off, size_t len) {
  sl.live_bytes -= std::min(sl.live_bytes, len);
  if (sl.live && --sl.live == 0) {
    sl.used = 0;
    sl.holes.clear();
  } else if (off + len == sl.used) {
    sl.used = off;
    if (!sl.holes.empty() && sl.holes.back().first + sl.holes.back().second == sl.used) {
      sl.used = sl.holes.back().first;
      sl.holes.pop_back();
    }
  } else {
    auto it = std::lower_bound(sl.holes.begin(), sl.holes.end(), std::make_pair(off, (size_t)0));
    it = sl.holes.insert(it, std::make_pair(off, len));
    if (it + 1 != sl.holes.end() && it->first + it->second == (it + 1)->first) {
      it->second += (it + 1)->second;
      it = sl.holes.erase(it + 1) - 1;
    }
    if (it != sl.holes.begin() && (it - 1)->first + (it - 1)->second == it->first) {
      (it - 1)->second += it->second;
      sl.holes.erase(it);
    }
  }
}

// the slabs' share of wbx_clip_pool_stats (the caller adds the clips with an allocation of their own to both)
inline void pool_slab_stats(const ClipSlabs& slabs, uint32_t* n_slabs, uint64_t* bytes_reserved, uint64_t* bytes_live) {
  uint64_t live = 0;
  for (auto& sl : slabs) live += sl->live_bytes;
  *n_slabs = (uint32_t)slabs.size();
  *bytes_reserved = pool_slab_bytes(slabs);
  *bytes_live = live;
}

}  // namespace wbx
