"""The clip pool's extent policy (whitebox_amd/csrc/wbx_pool.h) stated a second time, for tests/test_pool_model.py.
TEST INFRASTRUCTURE — nothing here is shipped.

Not a transcription: the header keeps a bump pointer and a sorted, merged hole list per slab; this model keeps ONE BITMAP
OF 64-KiB GRANULES per slab (1 = inside a live extent) and derives everything else from it:

  used       the end of the highest live extent, 0 for an empty slab
  a hole     a maximal run of free granules below `used`
  placement  from the newest slab to the oldest: the lowest maximal free run below `used` that is at least `need`,
             else that slab's tail [used, size) if it has room, else the next older slab; else a new slab
  new slab   max(64 MiB << 2 n_slabs — 1 GiB from the third slab on —, need); under a limit the usual size if
             reserved + size <= limit, else exactly `need`, else the request is refused.  Where the driver has no memory
             for the slab the clip gets an allocation of its own
  own        requests above 256 MiB never enter a slab; under a limit reserved + own_bytes must stay within it

and the three figures of wbx_clip_pool_stats: slabs, bytes reserved from the driver, bytes held by live clips.  Every
take and give also says WHICH case it was (a set of tags), for the census of the test's scripts."""
from __future__ import annotations

from typing import Dict, List, Optional, Set, Tuple

G = 64 << 10                 # granule
SLABBED = (256 << 20) // G   # granules of the largest request that is slabbed (a quarter of 1 GiB)
IN_SLAB, OWN, LIMIT = 0, 1, 2   # PoolWhere (wbx_pool.h)


def extent(nbytes: int, placed: int, jitter: bool = True) -> Tuple[int, int]:
    """(body, gap) in bytes of a clip whose channel rows take nbytes, the (placed + 1)-th clip of its context"""
    body = -(-nbytes // G)
    span = min(16, body // 8 + 1)
    gap = ((((placed + 1) * 2654435761) & 0xFFFFFFFF) >> 8) % span if jitter else 0
    return body * G, gap * G


class Slab:
    def __init__(self, granules: int):
        self.bits = bytearray(granules)
        self.ids: Set[int] = set()

    @property
    def size(self) -> int:
        return len(self.bits)

    @property
    def used(self) -> int:
        return self.bits.rfind(1) + 1

    def runs(self) -> List[Tuple[int, int]]:
        """the maximal free runs below `used`, (first granule, granules)"""
        out, p, used = [], 0, self.used
        while True:
            p = self.bits.find(0, p, used)
            if p < 0:
                return out
            q = self.bits.find(1, p)
            out.append((p, q - p))
            p = q


class PoolModel:
    def __init__(self):
        self.slabs: List[Slab] = []
        self.limit = 0
        self.driver_fails = False
        self.where: Dict[int, Tuple[int, int, int]] = {}   # id -> (slab index or -1, first granule, granules | own bytes)
        self.next_id = 0

    # ---- the figures of wbx_clip_pool_stats
    def own_bytes(self) -> int:
        return sum(n for s, _, n in self.where.values() if s < 0)

    def stats(self) -> Tuple[int, int, int]:
        own = self.own_bytes()
        return (len(self.slabs), sum(s.size for s in self.slabs) * G + own,
                sum(n for s, _, n in self.where.values() if s >= 0) * G + own)

    def reserved(self) -> int:
        return self.stats()[1]

    # ---- take
    def _book(self, si: int, at: int, need: int) -> int:
        s = self.slabs[si]
        assert not any(s.bits[at:at + need]) and at + need <= s.size, "the MODEL handed a granule out twice"
        s.bits[at:at + need] = b"\x01" * need
        i = self.next_id
        self.next_id += 1
        s.ids.add(i)
        self.where[i] = (si, at, need)
        return i

    def _own(self, own_bytes: int, tags: Set[str]):
        if self.limit and self.reserved() + own_bytes > self.limit:
            return LIMIT, None, -1, 0, tags | {"own_refused"}
        i = self.next_id
        self.next_id += 1
        self.where[i] = (-1, 0, own_bytes)
        return OWN, i, -1, 0, tags

    def take(self, need_bytes: int, own_bytes: int):
        """-> (where, id or None, slab index, offset in bytes, tags)"""
        assert need_bytes % G == 0 and need_bytes
        need = need_bytes // G
        if need > SLABBED:
            return self._own(own_bytes, {"own_big"})
        for si in reversed(range(len(self.slabs))):
            s = self.slabs[si]
            used = s.used
            at = s.bits.find(bytes(need), 0, used)   # the lowest run of `need` free granules starts a maximal run
            if at >= 0:
                tag = "hole_exact" if s.bits[at + need] else "hole_split"
                return IN_SLAB, self._book(si, at, need), si, at * G, {tag}
            if s.size - used >= need:
                return IN_SLAB, self._book(si, used, need), si, used * G, {"tail"}
        n = len(self.slabs)
        size = max(((64 << 20) << (2 * n)) // G if n < 2 else (1 << 30) // G, need)
        tags = {"slab_%d" % min(n + 1, 4)}
        if self.limit:
            tags.add("limit_usual")
            if self.reserved() + size * G > self.limit:
                size = need
                tags = tags - {"limit_usual"} | {"limit_exact"}
            if self.reserved() + size * G > self.limit:
                return LIMIT, None, -1, 0, {"limit_refused"}
        if self.driver_fails:
            return self._own(own_bytes, {"own_fallback"})
        self.slabs.append(Slab(size))
        return IN_SLAB, self._book(n, 0, need), n, 0, tags

    # ---- give
    def case_of(self, i: int) -> str:
        """which release an id would be: own / reset / newest / newest_hole / none / lower / upper / both"""
        si, at, n = self.where[i]
        if si < 0:
            return "own"
        s = self.slabs[si]
        if len(s.ids) == 1:
            return "reset"
        lower = at > 0 and not s.bits[at - 1]
        if at + n == s.used:
            return "newest_hole" if lower else "newest"
        upper = not s.bits[at + n]
        return {(0, 0): "none", (1, 0): "lower", (0, 1): "upper", (1, 1): "both"}[(int(lower), int(upper))]

    def give(self, i: int) -> str:
        case = self.case_of(i)
        si, at, n = self.where.pop(i)
        if si >= 0:
            s = self.slabs[si]
            s.bits[at:at + n] = bytes(n)
            s.ids.discard(i)
        return case

    def live_extents(self, si: int) -> List[Tuple[int, int]]:
        """(offset, bytes) of the live extents of a slab, sorted"""
        return sorted((at * G, n * G) for s, at, n in self.where.values() if s == si)

    def holes(self, si: int) -> List[Tuple[int, int]]:
        return [(p * G, n * G) for p, n in self.slabs[si].runs()]
