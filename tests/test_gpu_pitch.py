"""wbx_clip_pitch and wbx_engine_pitch_sample on the device.  Results come back through wbx_clip_download and are compared BIT
FOR BIT (uint32 views: -0.0 shows) with tests/pitch_model.py — the stretch's model to the intermediate length, then the
conversion's model of that intermediate —; the positions and the info are compared exactly, and every result keeps its
source's rate.  Sizes are the smallest at which the kernel can still go wrong: windows of 32, 64 and 256 frames (at N = 32 a
tile's span covers hundreds of steps, and steps straddle tile edges), results of one to six tiles that end inside a 16-byte
word, ranges shorter than a window, intermediates shorter than a step — and one call each across a band's seam of the
positions buffer."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import oracle_ffi as O
import pitch_model as M
import resample_model as RS
import second_pass as SP
import stretch_model as ST
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine, edit_desc

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 6000 + 300
SRC = {1: 1, 2: 2}                                              # channels -> clip id of a source
DST = 100
RATIOS = [(3, 2), (2, 3), (2, 1), (1, 2), (4, 1), (1, 4), (1265, 1194), (1194, 1265), (967, 1024)]
bits = BU.bits


def source(channels, n=SRC_LEN, seed=0x917, period=41.7):
    """seeded noise + a sine per channel (the channels at different periods)"""
    rng = np.random.default_rng(seed + channels)
    i = np.arange(n)
    return [(0.25 * rng.standard_normal(n) + np.sin(2 * np.pi * i / (period + 9 * c))).astype(np.float32) for c in range(channels)]


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
    yield c
    c.close()


def download(c, clip, channels, n):
    return [c.clip_download(clip, k, n, np.float32) for k in range(channels)]


def first_bad(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        if bad.size:
            return k, int(bad[0]), int(bad.size), g[bad[0]], w[bad[0]]
    return None


def check_stats(got, want, n, where):
    """wbx_clip_measure's rules: every field but sum / sum_sq exact, those two within any-order fp64 summation's bound"""
    assert FX.exact_fields_equal(got, want), (where, got, {k: want[k] for k in FX.EXACT})
    for k, mag in (("sum", "abs_sum"), ("sum_sq", "abs_sum_sq")):
        for g, w, a in zip(got[k], want[k], want[mag]):
            if np.isfinite(a):
                assert abs(g - w) <= n * 2.0 ** -52 * a, (where, k, g, w)


def launches_of(n, mid, N, D):
    """the kernel launches the header promises: per band of positions its search launches, and one more for the whole call"""
    L = W.lib()
    B, per, K = L.wbx_stretch_band_steps(), L.wbx_stretch_launch_steps(n, N, D), ST.steps(mid, N)
    return sum(-(-min(B, K - b) // per) for b in range(0, K, B)) + 1


def has_rate(c, clip, frames, rate):
    """layer 1 has no getter of a clip's rate; a conversion to the rate a clip has is refused as such, any other is not"""
    same = c.L.wbx_clip_resample(c.h, clip, 9000, 0, frames, rate, 1, None)
    msg = bytes(c.L.wbx_last_error(c.h))
    return same == -4 and b"that rate already" in msg


def run_and_check(c, clip, planes, first, n, m, num, den, q, N, D, dst=DST, stats=True, rate=RATE):
    """one call against the model: every position, the info, every output bit, the rate and stats_of_result.  Returns (the
    result's planes, the positions, the info)"""
    ch = len(planes)
    want, want_p, want_info = M.pitch_clip(planes, first, n, m, num, den, q, N, D)
    got = c.clip_pitch(clip, dst, first, n, m, num, den, q, N, D, positions=True, stats_channels=ch if stats else 0)
    info, pos = got[0], got[1]
    where = (ch, first, n, m, num, den, q, N, D)
    bad = np.flatnonzero(pos != want_p)
    assert pos.shape == want_p.shape and bad.size == 0, (where, "step", int(bad[0]), int(pos[bad[0]]), int(want_p[bad[0]]), bad.size)
    assert info == dict(want_info, launches=launches_of(n, want_info["mid_frames"], N, D)), (where, info, want_info)
    out = download(c, dst, ch, m)
    assert first_bad(out, want) is None, (where, first_bad(out, want))
    assert has_rate(c, dst, m, rate), where
    if stats:
        check_stats(got[2], FX.measure(want), m, where)
    return out, pos, info


# ---- 1: ratios x windows x tolerances x qualities, mono and stereo ----------------------------------------------------------------
def result_lengths(n):
    return [n, n + 1, n - 1, n // 2, 2 * n]


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: "%d-%d" % r)
@pytest.mark.parametrize("channels", [1, 2])
def test_pitch_matrix(ctx, channels, ratio):
    """every window and tolerance at one ratio; the quality, the range's length (700, 2100, 6000: results of one to six
    tiles) and the result's length (n, n +- 1, n / 2, 2 n) take turns, so each ratio meets every quality and every length.  The
    range starts inside the clip and, at the odd places, ends on its last frame"""
    num, den = ratio
    searched, seen_q, tiles = 0, set(), set()
    for i, (N, D) in enumerate((N, D) for N in (32, 64, 256) for D in (0, 8, 40)):
        q = (i + RATIOS.index(ratio)) % 3
        kind = (i + 2 * RATIOS.index(ratio)) % 5
        n = (700, 2100, 6000)[(i + i // 3) % 3]
        if kind == 4 and n == 6000:
            n = 3000                                            # twice 6000 would be twelve tiles
        m = result_lengths(n)[kind]
        first = SRC_LEN - n if i % 2 else (5, 0, 64)[i % 3]
        _, _, info = run_and_check(ctx, SRC[channels], ctx.src[channels], first, n, m, num, den, q, N, D)
        searched += info["searched_steps"]
        seen_q.add(q)
        tiles.add(-(-m // 1024))
    assert searched > 0 and seen_q == {0, 1, 2} and len(tiles) >= 3


def test_short_ranges_short_results_and_ragged_ends(ctx):
    """n < N, n = m = 1, an intermediate shorter than a step (m' < Hs), results that end inside a 16-byte word"""
    cases = ((10, 10, 3, 2, RS.FAST, 32, 8), (1, 1, 3, 2, RS.GOOD, 32, 0), (1, 1, 1, 2, RS.BEST, 32, 0), (1, 1, 4, 1, RS.FAST, 64, 3),
             (100, 7, 2, 1, RS.GOOD, 256, 40), (60, 13, 2, 3, RS.FAST, 64, 24), (500, 777, 967, 1024, RS.BEST, 64, 24),
             (333, 335, 1265, 1194, RS.GOOD, 48, 7), (2100, 4097, 1, 4, RS.FAST, 8192, 4096), (37, 70, 4, 1, RS.BEST, 32, 4),
             (31, 17, 1194, 1265, RS.FAST, 64, 24), (8, 2, 1, 2, RS.GOOD, 32, 3), (500, 1001, 2, 1, RS.FAST, 40, 20), (500, 1026, 1, 2, RS.GOOD, 32, 1))
    for ch in (1, 2):
        for n, m, num, den, q, N, D in cases:
            _, _, info = run_and_check(ctx, SRC[ch], ctx.src[ch], 7, n, m, num, den, q, N, D)
            assert info["mid_frames"] == M.mid_frames(m, num, den)
    assert any(M.mid_frames(m, num, den) < N // 2 for _, m, num, den, _, N, _ in cases) and any(m % 4 for _, m, *_ in cases)


# ---- 2: what the call reads --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_values_that_are_not_finite_and_frames_beside_the_range(channels):
    """The first tile's span starts below frame 0 of the intermediate and the last tile's ends past m': both are staged as
    zero and nothing is read for them.  Loud samples and NaNs in front of and behind the range, and in the pool's
    neighbours on both sides, do not count: the result is that of the range alone.  NaN and +-inf inside the range enter
    as 0.0"""
    c = W.MixContext(4, block=128)
    loud = [np.full(4096, 1e30, dtype=np.float32) for _ in range(channels)]
    for p in loud:
        p[::7] = np.nan
    planes = source(channels, 3000, seed=0xBE51DE)
    for k, p in enumerate(planes):
        p[:200], p[190:200], p[2700:], p[2710:2720] = 1e30, np.nan, -1e30, np.nan
        at = np.array([200, 205, 500, 1300, 1301, 2699]) - k * np.array([0, 1, 1, 1, 1, 1])
        p[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    planes[0].view(np.uint32)[240] = 0xFFC12345                 # a NaN with a payload and a sign
    planes[0][250] = np.float32(-0.0)
    c.clip_upload(53, "f32", RATE, loud)                        # the pool's neighbour in front ...
    c.clip_upload(54, "f32", RATE, planes)
    c.clip_upload(55, "f32", RATE, loud)                        # ... and behind
    for first, n in ((200, 2500), (200, 9), (2690, 10)):
        for m, num, den, q, N, D in ((n, 3, 2, RS.GOOD, 64, 24), (n // 2 + 1, 2, 3, RS.FAST, 32, 40), (n, 1265, 1194, RS.BEST, 256, 96),
                                     (2 * n + 3, 1, 2, RS.GOOD, 256, 96), (n, 4, 1, RS.FAST, 32, 8)):
            alone = [p[first:first + n].copy() for p in planes]
            want, want_p, _ = M.pitch_clip(alone, 0, n, m, num, den, q, N, D)
            assert np.all(np.isfinite(np.stack(want)))
            got, pos, _ = run_and_check(c, 54, planes, first, n, m, num, den, q, N, D)
            assert first_bad(got, want) is None and np.array_equal(pos, want_p)
    # the same with the range at the clip's two ends, the neighbours' frames right beside it
    edge = source(channels, 1500, seed=0xED6E)
    c.clip_upload(54, "f32", RATE, edge)
    for first, n in ((0, 1500), (0, 40), (1460, 40)):
        run_and_check(c, 54, edge, first, n, n, 2, 3, RS.BEST, 32, 8)
    c.close()


def test_silence_stays_silence(ctx):
    n = 2000
    for planes in ([np.zeros(n, dtype=np.float32)], [np.zeros(n, dtype=np.float32)] * 2):
        ctx.clip_upload(56, "f32", RATE, planes)
        for m, num, den, N, D in ((2000, 3, 2, 64, 24), (1300, 1194, 1265, 256, 96), (2500, 1, 4, 64, 40)):
            out, pos, info = run_and_check(ctx, 56, planes, 0, n, m, num, den, RS.GOOD, N, D)
            assert all(np.all(o.view(np.uint32) == 0) for o in out) and info["searched_steps"] > 0


# ---- 3: the composition, on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,dst_rate", [((3, 2), 32000), ((2, 3), 72000), ((2, 1), 24000), ((1, 2), 96000)], ids=lambda v: str(v))
def test_a_stretch_into_a_temporary_then_a_conversion_gives_the_same_frames(ctx, ratio, dst_rate):
    """what a caller had to do before, for the few ratios that have an integer rate: wbx_clip_stretch to m' frames into a
    temporary clip, then wbx_clip_resample.  Its first m frames are the pitch call's, bit for bit; only the rate differs"""
    num, den = ratio
    for ch in (1, 2):
        for n, m, q, N, D in ((2100, 2100, "good", 64, 24), (3000, 1501, "fast", 32, 8), (700, 1399, "best", 256, 40)):
            mid = W.pitch_mid_frames(m, num, den)
            pitched_info = ctx.clip_pitch(SRC[ch], 70, 11, n, m, num, den, q, N, D)
            stretched_info = ctx.clip_stretch(SRC[ch], 71, 11, n, mid, N, D)
            ctx.clip_resample(71, 72, 0, mid, dst_rate, q)
            total = W.resample_frames(RATE, dst_rate, mid)
            assert total >= m and pitched_info["mid_frames"] == mid
            assert {k: pitched_info[k] for k in ("steps", "searched_steps", "candidates", "max_shift")} == \
                   {k: stretched_info[k] for k in ("steps", "searched_steps", "candidates", "max_shift")}
            two_calls = [c[:m] for c in download(ctx, 72, ch, total)]
            assert first_bad(download(ctx, 70, ch, m), two_calls) is None, (ratio, ch, n, m)
            assert has_rate(ctx, 70, m, RATE) and has_rate(ctx, 72, total, dst_rate)


# ---- 4: the seams of the positions buffer ----------------------------------------------------------------------------------------
def test_a_call_across_a_search_launch_and_across_a_band_of_positions():
    """N = 32 and D = 4096, down an octave at eight times the length: K' = band_steps + 100, the intermediate four times the
    range (few steps search: the model stays quick).  Several search launches in the first band, one in the second; p, the
    counters and the positions cross both seams into ONE buffer"""
    L = W.lib()
    B = L.wbx_stretch_band_steps()
    mid = 16 * (B + 100) - 5
    m = 2 * mid
    n = -(-m // 8)
    assert W.pitch_mid_frames(m, 1, 2) == mid and ST.steps(mid, 32) == B + 100
    per = L.wbx_stretch_launch_steps(n, 32, 4096)
    assert 1 <= per < B
    c = W.MixContext(4, block=128)
    planes = source(1, n, seed=0x5EF)                           # (a step in some 340 searches; with this seed one of the last 100 does)
    c.clip_upload(1, "f32", RATE, planes)
    _, pos, info = run_and_check(c, 1, planes, 0, n, m, 1, 2, RS.FAST, 32, 4096, dst=2, stats=False)
    assert info["launches"] == -(-B // per) + 1 + 1 and info["searched_steps"] > 10
    searched = np.flatnonzero(np.diff(pos) != 16) + 1
    assert np.any(searched >= B) and np.any((searched > per) & (searched < B))
    c.close()


def test_a_band_seam_with_a_search_every_few_steps():
    """stereo, up a fifth at the range's own length with D = 24: the intermediate is 3/2 of the range, a step in nine
    searches, on both sides of the band's seam"""
    B = W.lib().wbx_stretch_band_steps()
    m = (16 * (B + 9) + 3) * 2 // 3
    mid = W.pitch_mid_frames(m, 3, 2)
    assert B + 9 <= ST.steps(mid, 32) <= B + 10
    c = W.MixContext(4, block=128)
    planes = source(2, m, seed=0x5EB)
    c.clip_upload(1, "f32", RATE, planes)
    _, pos, info = run_and_check(c, 1, planes, 0, m, m, 3, 2, RS.FAST, 32, 24, dst=2, stats=False)
    assert info["launches"] == launches_of(m, mid, 32, 24) >= 3 and info["searched_steps"] > B // 16
    searched = np.flatnonzero(np.diff(pos) != 16) + 1
    assert np.any(searched >= B) and np.any((searched > B - 40) & (searched < B))
    c.close()


def test_one_step_more_than_the_cap_is_refused_without_a_device_call(ctx):
    L = W.lib()
    cap = L.wbx_pitch_max_steps()
    mid = 16 * cap + 1                                          # K' = cap + 1 at N = 32
    before = ctx.pool_stats()
    pi = _ffi.PitchInfo()
    pi.steps = 777
    assert L.wbx_clip_pitch(ctx.h, SRC[1], DST + 1, 0, mid // 4, 2 * mid, 1, 2, 0, 32, 8, None, 0, C.byref(pi), None) == -3
    assert b"steps" in bytes(L.wbx_last_error(ctx.h)) and pi.steps == 777 and ctx.pool_stats() == before
    # ... one step fewer passes the sizes and fails on the clip, which is not that long
    assert L.wbx_clip_pitch(ctx.h, SRC[1], DST + 1, 0, mid // 4, 2 * (mid - 1), 1, 2, 0, 32, 8, None, 0, C.byref(pi), None) == -4
    assert b"past the clip" in bytes(L.wbx_last_error(ctx.h)) and ctx.pool_stats() == before


# ---- 4b: the second pass of pitch_kernel's grid -----------------------------------------------------------------------------------
class Intermediate:
    """one channel of the stretched intermediate, sliced lazily: ST.overlap_add over the steps a slice touches (and the one
    before them, whose frames are dropped: a step blends with its predecessor's position), on the frames of the range those
    steps read — `plane` may be lazy itself.  What lies past the range's n frames is zero, as in the model"""

    def __init__(self, plane, n, pos, N):
        self.plane, self.n, self.pos, self.N = plane, n, np.asarray(pos, dtype=np.int64), N

    def __getitem__(self, s):
        Hs = self.N // 2
        k0, k1 = s.start // Hs, -(-s.stop // Hs)
        assert s.step is None and 0 <= s.start <= s.stop and k1 <= len(self.pos)
        lead = 1 if k0 else 0
        p = self.pos[k0 - lead:k1]
        reads = np.concatenate([p, p[:-1] + Hs])                  # every step's own frames and its predecessor's continuation
        lo, hi = int(reads.min()), min(self.n, int(reads.max()) + Hs)
        x = ST.inputs([self.plane[lo:hi]])[0]
        y = ST.overlap_add([x], p - lo, (k1 - k0 + lead) * Hs, self.N)[0][lead * Hs:]
        return y[s.start - k0 * Hs:s.stop - k0 * Hs]


def export_window(c, clip, channels, j0, j1):
    """frames [j0, j1) of a resident clip as [channels] float32 planes, through wbx_clip_export (unclamped f32: the stored bits)"""
    out, _ = c.clip_export(clip, "f32", channels, j0, j1 - j0, clamp=False)
    return [np.ascontiguousarray(out.reshape(-1, channels)[:, k]) for k in range(channels)]


def test_the_lazy_intermediate_is_the_models():
    """(no device call) the windowed overlap-add equals ST.overlap_add of every step: at step seams, inside steps, where steps
    read past the range's end"""
    for n, mid, N in ((3000, 5000, 64), (700, 5003, 256), (5300, 5000, 64)):
        plane = source(1, n)[0]
        pos = np.array([ST.anchor(k, n, mid, N) for k in range(ST.steps(mid, N))], dtype=np.int32)
        pos[5:9] += [3, -2, 0, 7]                                 # steps moved off their anchors ...
        pos[7] = pos[6] + N // 2                                 # ... and one that continues its predecessor: a copy, no blend
        whole = ST.overlap_add(ST.inputs([plane]), pos, mid, N)[0]
        lazy = Intermediate(plane, n, pos, N)
        Hs = N // 2
        for a, b in ((0, 1), (0, 2 * Hs), (Hs - 1, Hs + 1), (Hs * 5 - 1, Hs * 9 + 2), (mid - 1000, mid), (mid - 10, mid)):
            assert np.array_equal(lazy[a:b].view(np.uint32), whole[a:b].view(np.uint32)), (n, mid, N, a, b)


@pytest.mark.parametrize("source_range,channels", [("eighth", 1), ("eighth", 2), ("longer", 2)])
def test_tiles_past_the_grid_cap(source_range, channels):
    """Down an octave (L 2, M 1: the tile is 1024) to G + 3 tiles, G the grid's cap (tests/second_pass.py, from
    wbx_pitch_launch_shape): workgroups 0, 1 and 2 stage and convert a second tile.  With D = 0 the positions are the anchors
    (test_stretch_host.py pins that for the model), so no search is modelled: the expected frames are ST.overlap_add over the
    steps a window's span touches, then the conversion's model of that window.  Compared bit for bit: the first three tiles,
    the frames around tile G's first, everything from tile G - 2 to the end — the whole second pass and the last lane's
    partial store (m = 1 mod 4).  From the "eighth" range, eight times shorter than the intermediate, the last step runs off
    the range's end after some 80 frames: most of the second pass stores silence.  From the "longer" range it blends frames of
    the range to the end, so a tile that is skipped or staged from the wrong step shows.  The same call at another quality
    is made and freed first: the memory the result then gets is not left as the driver handed it out"""
    n, m, mid, sh, G = SP.pitch_case(source_range)
    k = SP.PITCH
    num, den, q, N, D = k["num"], k["den"], k["quality"], k["window"], k["tolerance"]
    tile = sh["tile"]
    assert sh["n_tiles"] == G + 3 > sh["grid"] == G and m % 4 and q == "fast"
    K = ST.steps(mid, N)
    c = W.MixContext(4, block=128)
    seed, track, amp = 0x2D_9A55 + channels, 5, 0.75
    c.clip_synth(1, "f32", channels, RATE, n, seed, track, amp)
    c.clip_pitch(1, 2, 0, n, m, num, den, "good", N, D)         # fills the memory the result is about to get
    assert c.L.wbx_clip_free(c.h, 2) == 0
    info, pos = c.clip_pitch(1, 3, 0, n, m, num, den, q, N, D, positions=True)
    want_p = ((np.arange(K, dtype=np.int64) * (N // 2) * n) // mid).astype(np.int32)
    assert [int(want_p[j]) for j in (1, K // 2, K - 1)] == [ST.anchor(j, n, mid, N) for j in (1, K // 2, K - 1)]
    bad = np.flatnonzero(pos != want_p)
    assert pos.shape == want_p.shape and bad.size == 0, (bad[:8], bad.size)
    assert (info["steps"], info["mid_frames"], info["max_shift"], info["L"], info["M"]) == (K, mid, 0, 2, 1), info
    mids = [Intermediate(SP.SynthPlane(seed, track, ch, n, amp), n, want_p, N) for ch in range(channels)]
    tab = M.table(2, 1, RS.FAST)
    for j0, j1 in ((0, 3 * tile), (G * tile - 2048, G * tile + 2048), ((G - 2) * tile, m)):
        want = RS.resample(mids, 0, mid, num, den, RS.FAST, window=(j0, j1), tab=tab)
        if source_range == "longer":
            assert all(np.count_nonzero(w) > 0.99 * w.size for w in want), "the window holds signal, not silence"
        got = export_window(c, 3, channels, j0, j1)
        assert got[0].size == j1 - j0 and first_bad(got, want) is None, (j0, first_bad(got, want))
    c.close()


# ---- 5: around the call -----------------------------------------------------------------------------------------------------------
def test_no_intermediate_is_allocated_in_the_pool():
    """Up two octaves at the range's own length the intermediate has four times the result's frames.  Under a pool limit
    exactly as many results fit as plain copies of the range: nothing but the result is taken from the pool"""
    n = 1 << 19
    planes = source(2, n)

    def fill(make):
        c = W.MixContext(4, block=128)
        c.clip_upload(1, "f32", RATE, planes)                   # 4 MiB in the first slab (64 MiB)
        base = c.pool_stats()
        c.pool_limit(base[1])
        made = []
        while True:
            before = c.pool_stats()
            try:
                make(c, 10 + len(made))
            except W.WbxError as ex:
                assert ex.status == BU.OOM
                assert c.pool_stats() == before                 # the refused call changed nothing
                break
            made.append(10 + len(made))
            assert len(made) < 64
        return c, base, made

    c, base, made = fill(lambda c, dst: c.clip_pitch(1, dst, 0, n, n, 4, 1, "fast", 256, 0))
    c2, _, copies = fill(lambda c, dst: c.clip_derive(1, dst, edit_desc(0, n)))
    assert len(made) == len(copies) >= 2, (len(made), len(copies))
    c2.close()
    # D = 0 and a ratio of exactly 4: the anchors of the range's first 8192 frames alone are the same, a step reads nothing
    # beyond its anchor + N, and output j nothing beyond intermediate frame 4 j + H — the first 6000 frames are the model's
    want, _, _ = M.pitch_clip([p[:8192] for p in planes], 0, 8192, 8192, 4, 1, RS.FAST, 256, 0)
    got = [p[:6000] for p in download(c, made[-1], 2, n)]
    assert first_bad(got, [w[:6000] for w in want]) is None
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == base
    c.pool_limit(0)
    c.close()


def test_time_of_the_last_pitch_call_and_other_edits_caches():
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_pitch_ms(c.h, C.byref(out)) == -4 and out.value == 7.0       # none yet
    planes = source(1, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    assert c.L.wbx_pitch_ms(c.h, None) == -4
    c.clip_stretch(1, 3, 0, 5000, 7500, 256, 96)                # a stretch is no pitch call, nor a pitch call a stretch
    assert c.L.wbx_pitch_ms(c.h, C.byref(out)) == -4
    stretch_ms = c.stretch_ms()
    # the first pitch call of the context makes the conversion's table (no conversion has), and changes the cached window
    pit_want, _, _ = M.pitch_clip(planes, 0, 5000, 5000, 3, 2, RS.GOOD, 64, 24)
    c.clip_pitch(1, 4, 0, 5000, 5000, 3, 2, "good", 64, 24)
    assert 0.0 < c.pitch_ms() < 1000.0 and c.stretch_ms() == stretch_ms
    assert first_bad(download(c, 4, 1, 5000), pit_want) is None
    # a pitch call between two stretches of another window and between two conversions of its own plan leaves their
    # cached tables right; a stretch of the pitch call's window right behind it finds that window's table
    str_want, _, _ = ST.stretch_clip(planes, 0, 5000, 3333, 256, 96)
    str64_want, _, _ = ST.stretch_clip(planes, 0, 5000, 3333, 64, 24)
    rs_want = RS.resample(planes, 0, 5000, RATE, 32000, RS.GOOD)
    c.clip_stretch(1, 5, 0, 5000, 3333, 256, 96)
    c.clip_resample(1, 6, 0, 5000, 32000, "good")
    c.clip_pitch(1, 7, 0, 5000, 5000, 3, 2, "good", 64, 24)
    c.clip_stretch(1, 8, 0, 5000, 3333, 64, 24)
    c.clip_stretch(1, 9, 0, 5000, 3333, 256, 96)
    c.clip_resample(1, 10, 0, 5000, 32000, "good")
    c.clip_pitch(1, 11, 0, 5000, 5000, 3, 2, "good", 64, 24)
    for clip in (5, 9):
        assert first_bad(download(c, clip, 1, 3333), str_want) is None
    assert first_bad(download(c, 8, 1, 3333), str64_want) is None
    for clip in (6, 10):
        assert first_bad(download(c, clip, 1, len(rs_want[0])), rs_want) is None
    for clip in (7, 11):
        assert first_bad(download(c, clip, 1, 5000), pit_want) is None
    c.close()


def test_stats_of_result_equal_a_measure_of_the_result(ctx):
    for ch in (1, 2):
        _, _, stats = ctx.clip_pitch(SRC[ch], DST, 3, 2500, 2501, 1265, 1194, "good", 64, 24, positions=True, stats_channels=ch)
        measured = ctx.clip_measure(DST, ch, 0, 2501)
        assert FX.exact_fields_equal(stats, measured)
        for k in range(ch):                                     # the two sums within any-order fp64 summation's bound
            peak = float(measured["peak"][k])
            assert abs(stats["sum"][k] - measured["sum"][k]) <= 2501 * 2.0 ** -52 * 2501 * peak
            assert abs(stats["sum_sq"][k] - measured["sum_sq"][k]) <= 2501 * 2.0 ** -52 * 2501 * peak * peak


def test_a_replaced_dst_takes_the_old_extents_place_and_a_delete_restores_the_pool():
    c = W.MixContext(4, block=128)
    planes = source(2, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(2, "f32", RATE, [np.ones(4000, dtype=np.float32)] * 2)        # a neighbour behind what comes next
    base = c.pool_stats()
    c.clip_pitch(1, 10, 0, 3000, 4000, 3, 2, "fast", 64, 24)
    with_one = c.pool_stats()
    assert with_one[0] == base[0] and with_one[1] == base[1] and with_one[2] > base[2]
    for first in (5, 900):                                      # replaced by results of the same length: the same figures
        run_and_check(c, 1, planes, first, 3000, 4000, 3, 2, RS.FAST, 64, 24, dst=10)
        assert c.pool_stats() == with_one
    run_and_check(c, 1, planes, 0, 3000, 700, 2, 3, RS.FAST, 64, 24, dst=10)   # ... by a shorter one: nothing more is reserved or live
    assert c.pool_stats()[:2] == with_one[:2] and c.pool_stats()[2] <= with_one[2]
    assert all(np.all(p == 1.0) for p in download(c, 2, 2, 4000))
    assert c.L.wbx_clip_free(c.h, 10) == 0
    assert c.pool_stats() == base
    c.close()


def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    ctx.clip_pitch(SRC[2], DST, 0, 64, 96, 3, 2, "fast", 32, 8)
    kept = bits(np.stack(download(ctx, DST, 2, 96))).tolist()
    ctx.clip_upload(60, "i16", RATE, [np.arange(64, dtype=np.int16)] * 2)
    pi, st = _ffi.PitchInfo(), _ffi.ClipStats()
    pos = np.full(64, 9, dtype=np.int32)
    S = SRC[2]

    def refused(status, why, src=S, dst=DST, first=0, n=64, m=96, num=3, den=2, q=0, N=32, D=8, cap=None):
        before = ctx.pool_stats()
        pi.steps = 777
        got = L.wbx_clip_pitch(ctx.h, src, dst, first, n, m, num, den, q, N, D, None if cap is None else pos.ctypes.data, cap or 0,
                               C.byref(pi), C.byref(st))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 96))).tolist() == kept and pi.steps == 777
        assert np.all(pos == 9)

    refused(-4, b"unknown source", src=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"no frames", m=0)
    refused(-4, b"past the clip", first=SRC_LEN - 10, n=11, m=11)
    refused(-4, b"past the clip", first=(1 << 64) - 1, n=2, m=2)     # a sum that wraps
    refused(-4, b"may not replace", dst=S)
    refused(-4, b"term of 0", num=0)
    refused(-4, b"term of 0", den=0)
    refused(-4, b"ratio of 1", num=2)
    refused(-4, b"ratio of 1", num=960, den=960)
    refused(-4, b"unknown quality", q=3)
    refused(-4, b"unknown quality", q=-1)
    refused(-4, b"2^31 - 16", n=(1 << 30), m=(1 << 31) - 16)     # judged on the arithmetic: no clip is that long
    refused(-4, b"2^31 - 16", n=(1 << 30), m=(1 << 31) - 17)     # ... m passes, m' = 3 m / 2 does not: the stretch's refusal
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16, m=(1 << 30), num=2, den=3)
    for N in (0, 24, 36, 8200, 8192 + 8):
        refused(-4, b"window_frames", N=N)
    refused(-4, b"tolerance_frames", D=4097)
    refused(-4, b"positions_cap", cap=8)                        # m' = 144: K' = 9
    refused(-3, b"not F32", src=60)                             # (a clip of more than 2 channels cannot exist in the pool)
    refused(-3, b"two octaves", num=5, den=1)
    refused(-3, b"two octaves", num=1000, den=4001)
    refused(-3, b"1280 phases", num=1282, den=1281)
    refused(-3, b"ratio beyond 8", m=64 * 8 * 2 // 3 + 1)        # m' = 513 > 8 n
    refused(-3, b"ratio beyond 8", n=145 * 8, m=96)              # n > 8 m' = 1152
    refused(-3, b"two octaves", src=60, num=9, den=2)            # the sizes are judged before the clip is looked at
    refused(-4, b"window_frames", src=60, N=33)
    refused(-3, b"two octaves", num=5, den=1, N=33)              # ... and the ratio before the stretch's arguments
    refused(-4, b"past the clip", n=1 << 20, m=1 << 20)          # the sizes pass, the clip does not
    # what is not refused: the limits themselves, a capacity that is just enough
    got = L.wbx_clip_pitch(ctx.h, S, 62, SRC_LEN - 1, 1, 2, 4, 1, 2, 8192, 4096, pos.ctypes.data, 1, None, None)
    assert got == 0 and pos[0] == 0 and np.all(pos[1:] == 9)
    ctx.clip_pitch(S, 62, 0, 8 * 32, 128, 1, 4, "best", 32, 0)   # n = 8 m': the intermediate has 32 frames
    assert L.wbx_clip_free(ctx.h, 62) == 0


# ---- 6: through the engine -----------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_pitch_sample_and_transpose_sample_played_and_exported():
    spec = synth.make_session("pit2", 3, n_blocks=6, block=128, seed=0x917C2)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
    NU = 3000
    planes = source(2, NU + 8, seed=0x0B)
    up = eng.add_sample("f32", rate, planes)
    new, info = eng.pitch_sample(up, 1265, 1194, out_frames=4000, quality="good", window_frames=256, tolerance_frames=96, first_frame=4,
                                 n_frames=NU)
    want, _, want_info = M.pitch_clip(planes, 4, NU, 4000, 1265, 1194, RS.GOOD, 256, 96)
    assert eng._sample_shape[new] == (4000, 2) and {k: info[k] for k in want_info} == want_info and info["searched_steps"] > 0
    assert eng._sample_rate[new] == rate and first_bad(download(eng.ctx, new, 2, 4000), want) is None
    # up a fifth at the sample's own length: 40 ms and 10 ms at the sample's rate, on the interface's grid
    t_id, t_info = eng.transpose_sample(up, 7)
    num, den = W.pitch_ratio(7)
    N, D, m = 8 * int(round(40.0 * rate / 8000.0)), int(round(10.0 * rate / 1000.0)), NU + 8
    want_t, _, want_t_info = M.pitch_clip(planes, 0, m, m, num, den, RS.GOOD, N, D)
    assert abs(1200.0 * np.log2(num / den) - 700.0) < 0.4 and eng._sample_shape[t_id] == (m, 2)
    assert {k: t_info[k] for k in want_t_info} == want_t_info
    assert first_bad(download(eng.ctx, t_id, 2, m), want_t) is None

    # the transposed sample on a track at speed 1.0, against the oracle playing the MODEL's clip at the session's rate
    unit = BU.block_beats(spec.block, rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    for t in range(3):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
        while e.clips(t):
            e.delete_clip(t, 0)
    eng.add_audio_clip(eng.tracks[2], "pitched", 0.5 * unit, 5.5 * unit, 0.0, new, 1.0, 1.0)
    eng.add_audio_clip(eng.tracks[1], "transposed", 1.5 * unit, 4.5 * unit, 0.0, t_id, 1.0, 1.0)
    assert e.add_audio_clip(2, 0.5 * unit, 5.5 * unit, 0.0, oracle_sample(e, want, rate), 1.0, 1.0) == 0
    assert e.add_audio_clip(1, 1.5 * unit, 4.5 * unit, 0.0, oracle_sample(e, want_t, rate), 1.0, 1.0) == 0
    e.play()
    eng.play()
    eng.render(6)
    mm, _, _ = eng.ctx.fetch()
    heard = False
    for b in range(6):
        om, _ = e.process()
        assert np.array_equal(bits(mm[b]), bits(om)), b
        heard = heard or bool(om.any())
    assert heard
    got, _ = eng.export_sample(new, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(want, axis=1).reshape(-1).view(np.uint32))
    with pytest.raises(W.WbxError):
        eng.delete_sample(new)                                  # a clip names it
    spare, _ = eng.pitch_sample(up, 2, 3, window_frames=64, tolerance_frames=24)
    eng.delete_sample(spare)
    # refusals create no sample
    L, new_id = W.lib(), C.c_uint32(12345)
    call = lambda s, n, m, num=3, den=2, q=1, N=64, D=24, ref=C.byref(new_id): L.wbx_engine_pitch_sample(eng.h, s, 0, n, m, num, den, q, N, D,
                                                                                                        None, ref)
    assert call(9999, 8, 8) == -4
    assert call(spare, 8, 8) == -4                              # deleted
    assert call(up, NU + 9, NU) == -4
    assert call(up, 0, 8) == -4 and call(up, 8, 0) == -4
    assert call(up, 8, 8, num=0) == -4 and call(up, 8, 8, num=4, den=4) == -4 and call(up, 8, 8, q=5) == -4
    assert call(up, 8, 8, N=36) == -4 and call(up, 8, 8, D=4097) == -4
    assert call(up, 8, 8, num=9, den=2) == -3 and call(up, 8, 44) == -3 and call(up, 800, 60) == -3
    assert call(up, 8, 8, ref=None) == -4
    assert new_id.value == 12345
    assert call(up, NU + 8, NU) == 0 and new_id.value != 12345
    eng.close()
    e.close()


def test_cpp_adapter_transposes_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::pitch_sample; the result and the
    info equal the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_pitch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_pitch.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "pitched.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n = 5 * 512
    assert "adapter pitch ok %d" % n in out, out
    g = np.arange(n, dtype=np.uint64)
    ph = g % 50
    tri = np.where(ph < 25, ph, 50 - ph).astype(np.float32) / np.float32(32.0) - np.float32(0.375)
    x = tri + (((g * 2654435761) & 0xFFFFFFFF) >> 24).astype(np.float32) / np.float32(4096.0)
    want, _, info = M.pitch_clip([x.astype(np.float32)], 0, n, n, 3, 2, RS.GOOD, 256, 96)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == n and first_bad([got], want) is None
    assert ("steps %d searched %d candidates %d max_shift %d" % (info["steps"], info["searched_steps"], info["candidates"],
                                                                info["max_shift"])) in out and info["searched_steps"] > 0, out


# ---- 7: beside the audio thread -------------------------------------------------------------------------------------------------
def test_pitch_beside_the_audio_thread():
    """The shape of the stretch's test (test_gpu_stretch.py): a clip far behind the played range names the big source while
    the threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside one
    for the pin (-3, asked first) — one thread deletes without pause while the other transposes until a delete has been
    refused for the pin.  The master is what it is without the calls, and the last result equals the model."""
    NB, FR, WAIT, CALLS = 300, 1 << 19, 60.0, 96
    N, D = 1024, 512
    spec = synth.make_session("pitthr", 2, n_blocks=NB, block=128, seed=0x917712)
    planes = source(2, FR, seed=41, period=233.3)

    def with_big(eng):                                            # the same session in both runs
        sid = eng.add_sample("f32", 44100, planes)
        eng.add_audio_clip(eng.tracks[0], "far", 1000.0, 1001.0, 0.0, sid, 1.0, 1.0)
        return sid

    def run_blocks(eng, sink):
        out = W.AudioBuffer(spec.block, spec.channels)
        eng.play()
        for _ in range(NB):
            eng.process(None, out, float(spec.sample_rate))
            sink.append(np.stack(out.channel_buffers).copy())

    alone = []
    ref = build_engine(spec, max_blocks=1)
    with_big(ref)
    run_blocks(ref, alone)
    ref.close()

    eng = build_engine(spec, max_blocks=1)
    big = with_big(eng)
    first, n = 5, FR - 8
    L = W.lib()
    began, finished, refused = threading.Event(), threading.Event(), threading.Event()
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        while not finished.is_set() and time.monotonic() < end:
            st = L.wbx_engine_delete_sample(eng.h, big)
            key_ = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key_] = seen.get(key_, 0) + 1
            if st == -3:
                refused.set()

    def editor():
        try:
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["big"], results["info"] = eng.pitch_sample(big, 3, 2, quality="fast", window_frames=N, tolerance_frames=D,
                                                                   first_frame=first, n_frames=n, channels=2, frames=FR)
                results["calls"] += 1
        finally:
            began.set()
            finished.set()

    threads = [threading.Thread(target=f, args=a) for f, a in ((run_blocks, (eng, heard)), (deleter, ()), (editor, ()))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    assert len(heard) == NB and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(heard, alone))
    print("pitch calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    # every call read a live clip: the result is the model's, bit for bit
    want, _, want_info = M.pitch_clip(planes, first, n, n, 3, 2, RS.FAST, N, D)
    assert {k: results["info"][k] for k in want_info} == want_info and want_info["searched_steps"] > 100
    assert first_bad(download(eng.ctx, results["big"], 2, n), want) is None
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
