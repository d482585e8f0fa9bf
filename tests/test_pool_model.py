"""The clip pool's extent policy on the CPU: whitebox_amd/csrc/wbx_pool.h (through tests/cpp/pool_sim.cpp) against the
bitmap model of tests/pool_model.py, over seeded random scripts of take / give / replace — after EVERY operation the
placement, the three figures of wbx_clip_pool_stats and the slabs' books (hole list well formed; holes, live extents and
the tail partition the slab) — plus the two scenarios of test_gpu_parity.py's clip-storage tests, and the same header
stand-alone under ASan, UBSan and libstdc++'s debug mode (tests/cpp/pool_main.cpp)."""
from __future__ import annotations

import collections
import functools
import subprocess

import numpy as np
import pytest

import pool_model as PM
import pool_sim as PS
from pool_model import G

MENU = (1, 2, 3, 5, 8, 13, 40, 200,
        1024,    # the whole first slab
        4096,    # exactly a quarter slab: the largest request that is slabbed
        4097)    # an allocation of its own
# (weights over MENU, live extents aimed at)
PROFILES = {
    "small": ((6, 6, 6, 6, 6, 5, 4, 1, .15, .05, .05), 40),   # stays in a slab or two: holes, splits, merges
    "big": ((2, 2, 2, 2, 2, 2, 3, 4, 2, 1.5, 1), 14),         # slabs grow, empty, are reused
    "limit": ((2, 2, 2, 2, 2, 2, 4, 8, 3, 1, 1), 24),         # ... under wbx_clip_pool_limit, which moves
    "fail": ((2, 2, 2, 2, 2, 2, 3, 4, 2, 1.5, 1), 14),        # ... with a driver that is out of memory now and then
}
SEEDS = range(16)
N_OPS = 320
CASES = [(p, s) for p in PROFILES for s in SEEDS]
CENSUS_MIN = 20
CENSUS_KINDS = ("newest", "newest_hole", "lower", "upper", "both", "none", "reset", "own",   # releases
                "hole_exact", "hole_split", "tail", "slab_2", "slab_3",                        # placements
                "limit_usual", "limit_exact", "limit_refused", "own_refused",                  # each outcome of a limit
                "own_big", "own_fallback", "replace")


@functools.lru_cache(maxsize=None)
def make_script(profile: str, seed: int):
    """-> (ops, census).  ops: ("take", key, need, own_bytes) / ("give", key) / ("replace", new key, need, own_bytes, old
    key) / ("limit", bytes) / ("fails", bool); the last gives empty the pool.  The generator asks the model which release
    case every live extent would be, so that all of them come up; what the model ANSWERS is not part of the script."""
    rng = np.random.default_rng([0x9001, list(PROFILES).index(profile), seed])
    weights, target = PROFILES[profile]
    weights = np.array(weights) / sum(weights)
    m, ops, census = PM.PoolModel(), [], collections.Counter()
    ids = {}   # key -> model id
    keys = iter(range(1 << 30))

    def take(kind, old=None):
        need = int(MENU[rng.choice(len(MENU), p=weights)]) * G
        own = need - int(rng.integers(0, G))
        key = next(keys)
        census["size_%d" % (need // G)] += 1
        ops.append((kind, key, need, own) + (() if old is None else (old,)))
        where, i, _, _, tags = m.take(need, own)
        census.update(tags)
        if i is not None:
            ids[key] = i
        return i is not None

    def give(key):
        census[m.give(ids.pop(key))] += 1

    if profile == "limit":
        m.limit = int(rng.choice([(64 << 20) + 40 * G, (64 << 20) + 300 * G, (64 << 20) + 1500 * G, 320 << 20, (320 << 20) + 300 * G]))
        ops.append(("limit", m.limit))
    if profile == "fail" and seed % 2:
        m.driver_fails = True
        ops.append(("fails", True))
    while len(ops) < N_OPS:
        r = rng.random()
        if profile == "limit" and r < .06:
            m.limit = 0 if rng.random() < .15 else m.reserved() + int(rng.choice([0, 5, 40, 300, 300, 1500, 4096 + 100, 16384, 16384 + 4096])) * G
            ops.append(("limit", m.limit))
            continue
        if profile == "fail" and r < .04:
            m.driver_fails = not m.driver_fails
            ops.append(("fails", m.driver_fails))
            continue
        r = rng.random()
        if not ids or r < (.55 if len(ids) < target else .25):
            take("take")
        elif r < .85:   # a give: first the case, then one of its extents, so that the rare cases get their share
            by_case = collections.defaultdict(list)
            for key, i in ids.items():
                by_case[m.case_of(i)].append(key)
            case = sorted(by_case)[rng.integers(len(by_case))]
            key = by_case[case][rng.integers(len(by_case[case]))]
            ops.append(("give", key))
            give(key)
        else:           # replace-on-publish: the new clip is built, then the old one released
            old = list(ids)[rng.integers(len(ids))]
            if take("replace", old):
                census["replace"] += 1
                give(old)
    for key in [list(ids)[k] for k in rng.permutation(len(ids))]:
        ops.append(("give", key))
        give(key)
    return tuple(ops), census


def census():
    total = collections.Counter()
    for p, s in CASES:
        total.update(make_script(p, s)[1])
    return total


# (at import: a script set that lost a case must not pass for want of it)
_census = census()
assert all(_census[k] >= CENSUS_MIN for k in CENSUS_KINDS), {k: _census[k] for k in CENSUS_KINDS}
assert all(len(make_script(p, s)[0]) >= 300 for p, s in CASES)
assert all(_census["size_%d" % n] >= CENSUS_MIN for n in MENU), _census


def check_books(sim, model, live):
    """live: key -> (slab, offset, bytes) as the SIM placed them"""
    stats = sim.stats()
    assert stats == model.stats()
    for si in range(stats[0]):
        size, used, n_live, live_bytes, holes = sim.dump(si)
        extents = sorted((off, n) for s, off, n in live.values() if s == si)
        assert all(n > 0 for _, n in holes), holes
        assert all(a + n < b for (a, n), (b, _) in zip(holes, holes[1:])), f"unsorted, overlapping or adjacent holes {holes}"
        assert not holes or holes[-1][0] + holes[-1][1] < used, f"a hole reaches the bump pointer {used}: {holes}"
        pos = 0
        for off, n in sorted(holes + extents):   # holes and live extents tile [0, used); the tail is [used, size)
            assert off == pos, f"slab {si}: gap or overlap at {pos}: holes {holes}, extents {extents}"
            pos += n
        assert pos == used <= size
        assert (n_live, live_bytes) == (len(extents), sum(n for _, n in extents))
        assert (size, used) == (model.slabs[si].size * G, model.slabs[si].used * G)
        assert holes == model.holes(si) and extents == model.live_extents(si)


def replay(ops, sim, model, every_op=True):
    """-> the placements, one (where, slab, offset) per take"""
    live, sim_ids, model_ids, placed = {}, {}, {}, []

    def take(key, need, own):
        where, i, slab, off = sim.take(need, own)
        m_where, m_i, m_slab, m_off, _ = model.take(need, own)
        assert (where, slab, off) == (m_where, m_slab, m_off), f"take of {need // G} granules"
        placed.append((where, slab, off))
        if i is not None:
            sim_ids[key], model_ids[key] = i, m_i
            live[key] = (slab, off, need if where == PM.IN_SLAB else own)

    def give(key):
        sim.give(sim_ids.pop(key))
        model.give(model_ids.pop(key))
        del live[key]

    for n, op in enumerate(ops):
        if op[0] == "take":
            take(*op[1:])
        elif op[0] == "give":
            give(op[1])
        elif op[0] == "replace":
            take(*op[1:4])
            if every_op:
                check_books(sim, model, live)
            if op[1] in live:
                give(op[4])
        elif op[0] == "limit":
            sim.set_limit(op[1])
            model.limit = op[1]
        else:
            sim.set_driver_fails(op[1])
            model.driver_fails = op[1]
        if every_op:
            check_books(sim, model, live)
    check_books(sim, model, live)
    return placed, live


@pytest.mark.parametrize("profile,seed", CASES)
def test_random_scripts_place_every_extent_where_the_model_does(profile, seed):
    ops, _ = make_script(profile, seed)
    sim, model = PS.PoolSim(), PM.PoolModel()
    _, live = replay(ops, sim, model)
    assert not live                                     # everything was given back:
    n, _, bytes_live = sim.stats()
    assert bytes_live == 0
    for si in range(n):
        _, used, n_live, live_bytes, holes = sim.dump(si)
        assert (used, n_live, live_bytes, holes) == (0, 0, 0, [])
    sim.close()


def test_the_gap_in_front_of_a_clip():
    """pool_extent against the formula: body in whole granules, a gap of hash(placed + 1) mod min(16, body / 8 + 1)"""
    for nbytes in (1, G - 1, G, G + 1, 8 * G - 1, 8 * G, 8 * G + 1, 24 * G, 120 * G, 121 * G, 367 * G, 4096 * G, 5000 * G):
        spans = set()
        for placed in list(range(64)) + [0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF]:
            body, gap = PS.extent(nbytes, placed)
            assert (body, gap) == PM.extent(nbytes, placed)
            assert body % G == 0 and 0 <= body - nbytes < G and gap % G == 0 and gap // G < min(16, body // G // 8 + 1)
            spans.add(gap)
            assert PS.extent(nbytes, placed, jitter=False) == (body, 0)
        assert len(spans) == min(16, body // G // 8 + 1)   # every gap of the span comes up


def _clip_bytes(frames, channels, elem=4):
    return -(-(frames + 16) * elem // 256) * 256 * channels   # rows of frames + 16 padding frames, 256-B aligned


def _pair():
    return PS.PoolSim(), PM.PoolModel()


def test_replacing_a_shrinking_clip_beside_a_long_lived_one_stays_in_one_slab():
    """test_gpu_parity.test_clip_storage_reuses_the_extent_of_a_replaced_clip, its requests as clip_build makes them"""
    ops = [("take", 0) + _need(_clip_bytes(1_000_000, 1), 0)]
    for i in range(40):   # 40 x 16 MB through a 64-MiB slab
        need = _need(_clip_bytes(4_000_000 - 1000 * i, 1), 1 + i)
        ops.append(("take", 1, *need) if i == 0 else ("replace", 1 + i, *need, i))
    sim, model = _pair()
    placed, live = replay(ops, sim, model)
    assert all(where == PM.IN_SLAB and slab == 0 for where, slab, _ in placed)
    n, reserved, bytes_live = sim.stats()
    assert n == 1 and reserved == 64 << 20 and bytes_live < 24 << 20 and len(live) == 2
    sim.close()


def _need(nbytes, placed):
    body, gap = PM.extent(nbytes, placed)
    return body + gap, nbytes


def test_nine_24_mb_clips_spill_over_slabs():
    """test_gpu_parity.test_clip_storage_slabs_grow_and_are_reused: nine stereo clips, one of 320 MB, three freed and
    smaller ones uploaded in their place"""
    ops = [("take", k) + _need(_clip_bytes(3_000_000, 2), k) for k in range(9)]
    ops.append(("take", 9) + _need(_clip_bytes(80_000_000, 2, elem=2), 9))
    for n, k in enumerate((1, 4, 7)):
        ops += [("give", k), ("take", 10 + n) + _need(_clip_bytes(1_500_000, 1), 10 + n)]
    sim, model = _pair()
    placed, live = replay(ops, sim, model)
    assert [slab for _, slab, _ in placed[:9]] == [0, 0, 1, 1, 1, 1, 1, 1, 1]   # 367 granules + gap each: two per 64 MiB
    assert placed[9][0] == PM.OWN
    assert all(where == PM.IN_SLAB for where, _, _ in placed[10:])
    own = _clip_bytes(80_000_000, 2, elem=2)
    assert sim.stats()[:2] == (2, (320 << 20) + own) and len(live) == 10
    sim.close()


def script_text(ops, placed):
    """a script and the model's placements as tests/cpp/pool_main.cpp reads them"""
    out, it = [], iter(placed)
    for op in ops:
        if op[0] in ("take", "replace"):
            where, slab, off = next(it)
            out.append("T %d %d %d %d %d %d" % (op[1], op[2], op[3], where, slab, off))
            if op[0] == "replace" and where != PM.LIMIT:
                out.append("G %d" % op[4])
        elif op[0] == "give":
            out.append("G %d" % op[1])
        elif op[0] == "limit":
            out.append("L %d" % op[1])
        else:
            out.append("F %d" % int(op[1]))
    return "\n".join(out) + "\n"


def digest(placed):
    d = 0xCBF29CE484222325
    for where, slab, off in placed:
        for v in (where, slab + 1, off):
            d = ((d ^ v) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return d


def test_the_pool_header_under_sanitizers_and_debug_containers(tmp_path):
    """tests/cpp/pool_main.cpp: wbx_pool.h alone, stand-alone (its own main), two scripts of every profile with the
    invariants checked in C++ — under ASan, UBSan and _GLIBCXX_DEBUG, which is what sees an iterator used after erase"""
    exe = str(tmp_path / "pool_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D_GLIBCXX_DEBUG", PS.MAIN, "-o", exe])
    files, want = [], []
    for profile in PROFILES:
        for seed in (0, 1):
            ops, _ = make_script(profile, seed)
            model, placed = PM.PoolModel(), []
            ids = {}
            for op in ops:   # the model alone
                if op[0] in ("take", "replace"):
                    where, i, slab, off, _ = model.take(op[2], op[3])
                    placed.append((where, slab, off))
                    if i is not None:
                        ids[op[1]] = i
                        if op[0] == "replace":
                            model.give(ids.pop(op[4]))
                elif op[0] == "give":
                    model.give(ids.pop(op[1]))
                elif op[0] == "limit":
                    model.limit = op[1]
                else:
                    model.driver_fails = op[1]
            path = tmp_path / f"{profile}_{seed}.txt"
            path.write_text(script_text(ops, placed))
            files.append(str(path))
            want.append("%s_%d %d %016x" % (profile, seed, len(placed), digest(placed)))
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    assert out.stdout.strip().splitlines() == want
