"""wbx_clip_warp and wbx_engine_warp_sample on the device.  Results come back through wbx_clip_download and are compared BIT
FOR BIT (uint32 views: -0.0 shows) with tests/warp_model.py, the numpy twin of the header's text; the positions and the info
are compared exactly.  With no markers the call is compared with wbx_clip_stretch ON THE DEVICE as well.  Sizes are the
smallest at which the kernels can still go wrong: a few thousand frames, segments shorter than a hop, exactly a hop and a
hop plus one, markers one frame apart, results that end inside a 16-byte word — and one call each across a workgroup's launch
bound (rounds), across a launch's workgroup bound (slices), and with the widest span the search stages."""
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
import stretch_model as SM
import warp_model as M
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 20000 + 300
SRC = {1: 1, 2: 2}                                              # channels -> clip id of a source
DST = 100
bits = BU.bits


def source(channels, n=SRC_LEN, seed=0x3A9, period=41.7):
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


def launches_of(n, m, mk, N, D):
    return M.launches(n, m, mk, N, D, W.lib().wbx_warp_launch_segments())


def run_and_check(c, clip, planes, first, n, m, mk, N, D, dst=DST, stats=True):
    """one call against the model: every position, the info, every output bit and stats_of_result.  Returns (the result's
    planes, the positions, the info)"""
    ch = len(planes)
    assert M.check(n, m, mk, N, D) == 0, (n, m, mk, N, D)
    want, want_p, want_info = M.warp_clip(planes, first, n, m, mk, N, D)
    got = c.clip_warp(clip, dst, first, n, m, mk, N, D, positions=True, stats_channels=ch if stats else 0)
    info, pos = got[0], got[1]
    where = (ch, first, n, m, len(mk), N, D)
    bad = np.flatnonzero(pos != want_p)
    assert bad.size == 0, (where, "step", int(bad[0]), int(pos[bad[0]]), int(want_p[bad[0]]), bad.size)
    assert info == dict(want_info, launches=launches_of(n, m, mk, N, D)), (where, info, want_info)
    assert info["launches"] == W.warp_launches(n, m, mk, N, D)
    out = download(c, dst, ch, m)
    assert first_bad(out, want) is None, (where, first_bad(out, want))
    if stats:
        check_stats(got[2], FX.measure(want), m, where)
    return out, pos, info


# ---- 1: no markers: the call IS wbx_clip_stretch ------------------------------------------------------------------------------
def lengths(n):
    return [-(-n // 8), 2 * n // 3, n - 1, n + 1, 3 * n // 2, 8 * n]     # (an eighth rounded up: 8 m >= n)


@pytest.mark.parametrize("D", [0, 1, 24, 40])
@pytest.mark.parametrize("N", [32, 64, 256])
@pytest.mark.parametrize("channels", [1, 2])
def test_without_markers_the_call_is_the_stretch_on_the_device(ctx, channels, N, D):
    n = 2100
    searched = 0
    for i, m in enumerate(lengths(n)):
        first = SRC_LEN - n if i % 2 else (5, 0, 64)[i % 3]
        out, pos, info = run_and_check(ctx, SRC[channels], ctx.src[channels], first, n, m, [], N, D, stats=False)
        s_info, s_pos = ctx.clip_stretch(SRC[channels], DST + 1, first, n, m, N, D, positions=True)
        assert np.array_equal(pos, s_pos) and all(info[k] == s_info[k] for k in ("steps", "searched_steps", "candidates", "max_shift"))
        assert first_bad(out, download(ctx, DST + 1, channels, m)) is None, (channels, N, D, m)
        assert info["segments"] == 1 and info["longest_segment_steps"] == info["steps"]
        searched += info["searched_steps"]
    assert searched > 0 or D == 1


# ---- 2: markers -----------------------------------------------------------------------------------------------------------------
def seeded_markers(rng, n, M_, spread=3.0):
    """M_ strictly ascending pairs with segment ratios within `spread`; returns (markers, m)"""
    s = np.sort(rng.choice(np.arange(1, n), M_, replace=False)).tolist()
    out, last = [], (0, 0)
    for a in s + [n]:
        d = a - last[0]
        t = last[1] + int(rng.integers(max(1, int(np.ceil(d / spread))), max(1, int(d * spread)) + 1))
        out.append((a, t))
        last = (a, t)
    return out[:-1], out[-1][1] | 1                               # (an odd result: it ends inside a 16-byte word)


@pytest.mark.parametrize("M_", [1, 3, 17])
@pytest.mark.parametrize("shape", [(1, 32, 8), (2, 64, 40), (2, 256, 24), (1, 256, 96)], ids=lambda s: "ch%d-N%d-D%d" % s)
def test_seeded_markers(ctx, shape, M_):
    ch, N, D = shape
    rng = np.random.default_rng(0xBEA7 + 131 * M_ + N + D)
    n = int(rng.integers(3000, 20001))
    mk, m = seeded_markers(rng, n, M_)
    first = int(rng.integers(0, SRC_LEN - n + 1))
    _, _, info = run_and_check(ctx, SRC[ch], ctx.src[ch], first, n, m, mk, N, D)
    assert info["segments"] == M_ + 1 and info["searched_steps"] > 0 and (M_ == 1 or any(t % 4 for _, t in mk))


def test_short_segments_adjacent_markers_extreme_ratios_and_markers_at_the_ends(ctx):
    """segments shorter than a hop, exactly a hop and a hop plus one; markers 1 frame apart in either column; a segment at
    ratio 8 beside one at 1 / 8; a marker in the last 3 frames of the range and of the result"""
    for ch, N, D in ((1, 32, 8), (2, 64, 24), (2, 256, 40)):
        Hs = N // 2
        n = 6000
        mk = [(300, 300),
              (300 + Hs, 300 + Hs - 1),                          # m_j = Hs - 1: shorter than a hop
              (300 + 2 * Hs, 300 + 2 * Hs - 1),                  # m_j = Hs
              (300 + 3 * Hs, 300 + 3 * Hs),                      # m_j = Hs + 1
              (301 + 3 * Hs, 300 + 3 * Hs + 5),                  # 1 source frame into 5
              (308 + 3 * Hs, 300 + 3 * Hs + 6),                  # 7 source frames into 1: adjacent in the output column
              (309 + 3 * Hs, 300 + 3 * Hs + 7),                  # 1 into 1: adjacent in both
              (1500, 1500 + Hs - 3)]
        t = mk[-1][1]
        mk += [(1500 + 100, t + 800), (1500 + 100 + 800, t + 900)]          # ratio 8, then ratio 1 / 8
        mk += [(2400 + 5, t + 900 + 5 - 2)]                      # m_j = 3: shorter than a hop
        mk += [(n - 2, t + 5000)]                                # in the last 3 frames of the range ...
        m = t + 5002                                             # ... and of the result
        _, pos, info = run_and_check(ctx, SRC[ch], ctx.src[ch], 11, n, m, mk, N, D)
        segs = M.segments(n, m, mk, N)
        assert [g[3] for g in segs[1:4]] == [1, 1, 2] and segs[-1][3] == 1 and info["segments"] == len(mk) + 1
        assert all(pos[g[2]] == g[0] for g in segs)               # every pinned step


def test_a_template_past_the_ranges_end_and_candidates_across_a_marker(ctx):
    """the range ends loud and is stretched eightfold behind a marker: the last continuations start behind the range's end,
    their template is all zeros and the step takes lo; a tolerance wider than the neighbouring segments lets candidates lie
    beyond markers on both sides"""
    for ch in (1, 2):
        n, N, D = 1800, 256, 24
        planes = [p.copy() for p in ctx.src[ch]]
        for p in planes:
            p[5 + n - 200:5 + n] *= np.float32(3.0)
        ctx.clip_upload(50, "f32", RATE, planes)
        mk = [(900, 700)]
        m = 700 + 8 * 900
        _, pos, _ = run_and_check(ctx, 50, planes, 5, n, m, mk, N, D)
        assert np.any(pos[1:] + N // 2 >= n)                     # a continuation behind the end
        mk = [(500, 640), (560, 720), (700, 800), (760, 1000)]   # segments of 60 .. 140 source frames, D = 96
        _, pos, info = run_and_check(ctx, 50, planes, 5, n, 2001, mk, 64, 96)
        segs = M.segments(n, 2001, mk, 64)
        crossed = [int(q) for g, nxt in zip(segs[1:4], segs[2:5]) for q in pos[g[2]:g[2] + g[3]] if q >= nxt[0] or q < g[0]]
        assert crossed and info["searched_steps"] > 0, "no position lies beyond its segment's markers"


def test_non_finite_samples_silence_opposite_channels_and_ties(ctx):
    n = 4000
    mk = [(700, 1001), (1900, 2003), (2500, 3301)]
    m = 5003
    planes = [p[:n + 20].copy() for p in ctx.src[2]]
    for p, v in zip(planes, (np.nan, np.inf)):                   # NaN / +-inf inside the range, loud samples beside it
        p[[10, 700, 1901, n - 1]] = np.float32(v)
        p[2000:2040] = np.float32(-np.inf)
        p[:10] = np.float32(1e30)
        p[10 + n:] = np.float32(-1e30)
    ctx.clip_upload(51, "f32", RATE, planes)
    out, _, _ = run_and_check(ctx, 51, planes, 10, n, m, mk, 64, 24)
    assert all(np.all(np.isfinite(o)) for o in out)
    loud = ctx.src[1][0][:n]
    period8 = np.tile(np.array([0, 3, 5, 2, -1, -4, -2, 1], dtype=np.float32) / np.float32(4.0), n // 8)
    for planes in ([np.zeros(n, dtype=np.float32)], [loud, -loud], [period8], [period8, period8]):
        ctx.clip_upload(52, "f32", RATE, planes)
        for N, D in ((64, 24), (32, 40)):
            _, pos, info = run_and_check(ctx, 52, planes, 0, n, m, mk, N, D)
            assert info["searched_steps"] > 0                     # (silence and L = -R: every score 0, the lowest candidate)


def test_moving_an_earlier_marker_leaves_later_segments_positions(ctx):
    n, m, N, D = 9000, 11001, 64, 24
    base = [(2000, 2500), (4100, 5003), (7000, 8001)]
    _, p0, _ = run_and_check(ctx, SRC[2], ctx.src[2], 3, n, m, base, N, D, stats=False)
    moved = [(2100, 2400), (4100, 5003), (7000, 8001)]
    info, p1 = ctx.clip_warp(SRC[2], DST, 3, n, m, moved, N, D, positions=True)
    s0, s1 = M.segments(n, m, base, N), M.segments(n, m, moved, N)
    for j in (2, 3):
        assert s0[j][3] == s1[j][3] and np.array_equal(p0[s0[j][2]:s0[j][2] + s0[j][3]], p1[s1[j][2]:s1[j][2] + s1[j][3]])
    assert info["segments"] == 4


def click_take():
    """nine clicks on a noise floor; each should land on an odd target"""
    N, D = 256, 64
    rng = np.random.default_rng(0xC11C)
    ratios = [0.87, 1.25, 1.0, 0.93, 1.1, 1.21, 0.9, 1.05, 1.17, 1.0]
    events = [1500 + 1600 * i for i in range(9)]
    n = events[-1] + 1700
    x = (0.01 * rng.standard_normal(n)).astype(np.float32)
    for e in events:
        x[e:e + 40] += (np.exp(-np.arange(40) / 8.0) * np.cos(np.arange(40) * 0.9)).astype(np.float32)
    targets, t, s_prev = [], 0, 0
    for e, r in zip(events, ratios):
        t = t + int(round((e - s_prev) / r)) | 1
        targets.append(t)
        s_prev = e
    m = targets[-1] + int(round((n - events[-1]) / ratios[-1]))
    return [x], n, m, events, targets, N, D


def test_markers_a_hop_early_keep_every_click_intact(ctx):
    src, n, m, events, targets, N, D = click_take()
    Hs = N // 2
    mk = [(e - Hs, t - Hs) for e, t in zip(events, targets)]
    ctx.clip_upload(53, "f32", RATE, src)
    out, pos, info = run_and_check(ctx, 53, src, 0, n, m, mk, N, D)
    for e, t in zip(events, targets):
        assert np.array_equal(out[0][t:t + Hs].view(np.uint32), src[0][e:e + Hs].view(np.uint32)), (e, t)
    assert all(t % 4 for t in targets) and info["segments"] == 10


# ---- 3: rounds, slices, the widest step, the step limit -----------------------------------------------------------------------
def test_a_segment_longer_than_one_workgroups_launch_walks_in_rounds():
    """N = 32, D = 4096 on a range of 30 000: one segment has more steps than wbx_stretch_launch_steps says, beside short
    ones; compared at every step, the first and last of every round among them"""
    L = W.lib()
    n, N, D = 30000, 32, 4096
    Sr = L.wbx_stretch_launch_steps(n, N, D)
    long_m = (Sr + 900) * 16
    mk = [(200, 100), (400, 333), (400 + long_m // 8 + 50, 333 + long_m)]
    m = mk[-1][1] + 3000
    assert M.rounds(n, m, mk, N, D) == [4, 1]
    c = W.MixContext(4, block=128)
    planes = source(1, n, seed=0x50D)
    c.clip_upload(1, "f32", RATE, planes)
    _, pos, info = run_and_check(c, 1, planes, 0, n, m, mk, N, D, dst=2, stats=False)
    assert info["launches"] == 3 == W.warp_launches(n, m, mk, N, D) and info["longest_segment_steps"] == Sr + 900
    base = M.segments(n, m, mk, N)[2][2]
    want_p, _ = M.positions(SM.detector(SM.inputs(planes)), m, mk, N, D)
    for i in (0, 1, Sr - 1, Sr, Sr + 1, Sr + 899):              # the first and last step of either round (all steps were compared)
        assert pos[base + i] == want_p[base + i]
    chain = want_p[base:base + Sr + 900].astype(np.int64)
    left = np.flatnonzero(chain[1:] != chain[:-1] + 16) + 1     # the steps that left their continuation: they searched
    assert np.any(left < Sr) and np.any(left >= Sr), "a search in either round"
    c.close()


def test_more_segments_than_one_launch_takes_are_cut_into_slices():
    LS = W.lib().wbx_warp_launch_segments()
    S = LS + 5
    rng = np.random.default_rng(0x511CE)
    m_j = rng.integers(20, 51, S)
    n_j = np.maximum(1, (m_j * rng.uniform(0.7, 1.4, S)).astype(np.int64))
    s, t = np.cumsum(n_j), np.cumsum(m_j)
    mk = [(int(a), int(b)) for a, b in zip(s[:-1], t[:-1])]
    n, m = int(s[-1]), int(t[-1])
    c = W.MixContext(4, block=128)
    planes = source(2, n, seed=0x51)
    c.clip_upload(1, "f32", RATE, planes)
    _, _, info = run_and_check(c, 1, planes, 0, n, m, mk, 32, 8, dst=2)
    assert info["segments"] == S and info["launches"] == 3
    c.close()


def test_the_widest_step_in_a_two_segment_call(ctx):
    """N = 8192, D = 4096 on 20 000 frames: a searched step scores 8193 candidates over 4096 terms, three passes"""
    n, m = 20000, 38001
    mk = [(9000, 20001)]
    _, _, info = run_and_check(ctx, SRC[2], ctx.src[2], 100, n, m, mk, 8192, 4096)
    assert info["candidates"] >= 8193 and info["searched_steps"] >= 1


def test_one_step_past_the_step_limit_is_refused(ctx):
    L = W.lib()
    m = (1 << 22) * 16 + 1
    before = ctx.pool_stats()
    assert L.wbx_clip_warp(ctx.h, SRC[1], DST + 2, 0, m, m, None, 0, 32, 0, None, 0, None, None) == -3
    assert b"2^22 steps" in bytes(L.wbx_last_error(ctx.h)) and ctx.pool_stats() == before


# ---- 4: around the call -----------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_pool_outputs_and_dst_alone(ctx):
    L = W.lib()
    ctx.clip_warp(SRC[2], DST, 0, 64, 96, [(30, 40)], 32, 8)
    kept = bits(np.stack(download(ctx, DST, 2, 96))).tolist()
    ctx.clip_upload(60, "i16", RATE, [np.arange(64, dtype=np.int16)] * 2)
    wi, st = _ffi.WarpInfo(), _ffi.ClipStats()
    pos = np.full(64, 9, dtype=np.int32)
    S = SRC[2]

    def refused(status, why, src=S, dst=DST, first=0, n=64, m=96, mk=((30, 40),), N=32, D=8, cap=None, M_=None):
        before = ctx.pool_stats()
        wi.steps = 777
        arr = (_ffi.WarpMarker * max(1, len(mk)))()
        for i, (a, b) in enumerate(mk):
            arr[i].src_frame, arr[i].out_frame = a, b
        got = L.wbx_clip_warp(ctx.h, src, dst, first, n, m, None if not len(mk) else arr, len(mk) if M_ is None else M_, N, D,
                              None if cap is None else pos.ctypes.data, cap or 0, C.byref(wi), C.byref(st))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 96))).tolist() == kept and wi.steps == 777
        assert np.all(pos == 9)

    refused(-4, b"unknown source", src=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"no frames", m=0)
    refused(-4, b"past the clip", first=SRC_LEN - 10, n=41, m=41, mk=())
    refused(-4, b"may not replace", dst=S)
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16, m=(1 << 31) - 17)
    for N in (0, 24, 36, 8200):
        refused(-4, b"window_frames", N=N)
    refused(-4, b"tolerance_frames", D=4097)
    refused(-4, b"markers is NULL", mk=(), M_=1)
    refused(-4, b"65535", M_=65536)
    for mk in (((0, 40),), ((30, 0),), ((64, 90),), ((30, 96),), ((30, 40), (30, 50)), ((30, 40), (40, 40)), ((30, 40), (29, 50))):
        refused(-4, b"strictly ascending", mk=mk)
    refused(-4, b"positions_cap", cap=6)                        # K = 3 + 4
    refused(-3, b"ratio", mk=((2, 17),))
    refused(-3, b"ratio", mk=((33, 4),))
    refused(-3, b"ratio", mk=((60, 60),), m=96 + 0, n=64 + 300, first=0)      # the last segment: 304 source frames into 36
    refused(-3, b"not F32", src=60)
    refused(-3, b"ratio", src=60, n=1 << 20, m=1 << 10, mk=())   # the sizes are judged before the clip is looked at
    refused(-4, b"strictly ascending", src=60, mk=((0, 5),))
    refused(-4, b"past the clip", n=1 << 20, m=1 << 20, mk=())
    # what is not refused: a capacity that is just enough
    got = L.wbx_clip_warp(ctx.h, S, 62, 0, 64, 96, None, 0, 32, 8, pos.ctypes.data, 6, None, None)
    assert got == 0 and pos[0] == 0 and np.all(pos[6:] == 9)
    assert L.wbx_clip_free(ctx.h, 62) == 0


def test_pool_figures_the_pool_limit_and_the_time_of_the_last_call():
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_warp_ms(c.h, C.byref(out)) == -4 and out.value == 7.0        # none yet
    planes = source(2, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(2, "f32", RATE, [np.ones(4000, dtype=np.float32)] * 2)        # a neighbour behind what comes next
    c.clip_stretch(1, 9, 0, 3000, 4000, 64, 24)                 # a stretch is no warp call ...
    assert c.L.wbx_warp_ms(c.h, C.byref(out)) == -4 and c.L.wbx_warp_ms(c.h, None) == -4
    assert c.L.wbx_clip_free(c.h, 9) == 0
    base = c.pool_stats()
    mk = [(1000, 1500), (2000, 2600)]
    c.clip_warp(1, 10, 0, 3000, 4000, mk, 64, 24)
    assert 0.0 < c.warp_ms() < 1000.0
    with_one = c.pool_stats()
    assert with_one[0] == base[0] and with_one[1] == base[1] and with_one[2] > base[2]
    for first in (5, 900):                                      # replaced by results of the same length: the same figures
        run_and_check(c, 1, planes, first, 3000, 4000, mk, 64, 24, dst=10)
        assert c.pool_stats() == with_one
    # a stretch between two warps of one window leaves the cached window table valid, and the other way round
    want_s, _, _ = M.SM.stretch_clip(planes, 0, 3000, 4000, 64, 24)
    c.clip_stretch(1, 11, 0, 3000, 4000, 64, 24)
    run_and_check(c, 1, planes, 0, 3000, 700, [(1000, 300)], 64, 24, dst=10)   # a shorter one: nothing more is reserved or live
    assert first_bad(download(c, 11, 2, 4000), want_s) is None
    assert c.L.wbx_clip_free(c.h, 11) == 0
    assert c.pool_stats()[:2] == with_one[:2] and c.pool_stats()[2] <= with_one[2]
    assert all(np.all(p == 1.0) for p in download(c, 2, 2, 4000))
    assert c.L.wbx_clip_free(c.h, 10) == 0
    assert c.pool_stats() == base
    # the pool limit: a call that does not fit is refused with nothing left behind
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    n = 1 << 19
    big = source(2, n)
    c.clip_upload(3, "f32", RATE, big)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_warp(3, 20 + len(made), 0, n, 2 * n, [(n // 2, n)], 32, 0)     # 8 MiB each
        except W.WbxError as ex:
            assert ex.status == BU.OOM and c.pool_stats() == before
            break
        made.append(20 + len(made))
        assert len(made) < 64
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    c.pool_limit(0)
    c.close()


# ---- 5: through the engine -----------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_warp_sample_warp_to_markers_and_quantize_played_and_exported():
    spec = synth.make_session("wrp2", 3, n_blocks=6, block=128, seed=0x3A92)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
    NU = 3000
    planes = source(2, NU + 8, seed=0x0B)
    up = eng.add_sample("f32", rate, planes)
    mk = [(700, 1001), (1900, 2502)]
    new, info = eng.warp_sample(up, 4001, mk, 256, 96, first_frame=4, n_frames=NU)
    want, _, want_info = M.warp_clip(planes, 4, NU, 4001, mk, 256, 96)
    assert eng._sample_shape[new] == (4001, 2) and {k: info[k] for k in want_info} == want_info and info["searched_steps"] > 0
    assert first_bad(download(eng.ctx, new, 2, 4001), want) is None
    # events to targets, a hop early; pairs that break a rule are dropped, and the samples are the model's for what is reported
    events, targets = [400, 900, 905, 1500, 2990, 2600], [500, 880, 700, 1700, 2995, 20]
    w_id, w_info, used = eng.warp_to_markers(up, events, targets, window_frames=64, tolerance_frames=24)
    assert used == [(400 - 32, 500 - 32), (900 - 32, 880 - 32), (1500 - 32, 1700 - 32), (2990 - 32, 2995 - 32)]
    want_w, _, want_w_info = M.warp_clip(planes, 0, NU + 8, NU + 8, used, 64, 24)
    assert {k: w_info[k] for k in want_w_info} == want_w_info and first_bad(download(eng.ctx, w_id, 2, NU + 8), want_w) is None
    # quantize: onsets moved to a grid of 60 rate / (bpm division) frames, at the sample's own length
    click = np.zeros(24000, dtype=np.float32)
    rng = np.random.default_rng(5)
    click += (0.001 * rng.standard_normal(24000)).astype(np.float32)
    for at in (3100, 9000, 15300, 20800):
        click[at:at + 200] += (np.exp(-np.arange(200) / 40.0) * np.sin(np.arange(200) * 0.4)).astype(np.float32)
    cid = eng.add_sample("f32", rate, [click])
    q_id, q_info, q_used = eng.quantize_sample(cid, 120.0, division=4, window_frames=256, tolerance_frames=64)
    rec, _ = eng.onsets_sample(cid)
    grid = 60.0 * rate / (120.0 * 4)
    ev = [int(h) * 256 for h in np.flatnonzero(rec["onset"])]
    assert len(ev) >= 2 and len(q_used) >= 2 and set(q_used) <= {(e - 128, int(round(round(e / grid) * grid)) - 128) for e in ev}
    want_q, _, want_q_info = M.warp_clip([click], 0, 24000, 24000, q_used, 256, 64)
    assert {k: q_info[k] for k in want_q_info} == want_q_info and first_bad(download(eng.ctx, q_id, 1, 24000), want_q) is None
    eng.delete_sample(q_id)

    # the warped sample on a track at speed 1.0, against the oracle playing the MODEL's clip
    unit = BU.block_beats(spec.block, rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    for t in range(3):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
        while e.clips(t):
            e.delete_clip(t, 0)
    eng.add_audio_clip(eng.tracks[2], "warped", 0.5 * unit, 5.5 * unit, 0.0, new, 1.0, 1.0)
    assert e.add_audio_clip(2, 0.5 * unit, 5.5 * unit, 0.0, oracle_sample(e, want, rate), 1.0, 1.0) == 0
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
    eng.delete_sample(w_id)
    # refusals create no sample
    L, new_id = W.lib(), C.c_uint32(12345)
    arr = (_ffi.WarpMarker * 1)()
    arr[0].src_frame, arr[0].out_frame = 4, 5
    call = lambda s, n, m, N=64, D=24, M_=1, ref=C.byref(new_id): L.wbx_engine_warp_sample(eng.h, s, 0, n, m, arr, M_, N, D, None, ref)
    assert call(9999, 8, 8) == -4
    assert call(w_id, 8, 8) == -4                               # deleted
    assert call(up, NU + 9, NU) == -4
    assert call(up, 0, 8) == -4 and call(up, 8, 0) == -4
    assert call(up, 8, 8, N=36) == -4 and call(up, 8, 8, D=4097) == -4
    assert call(up, 4, 8) == -4 and call(up, 8, 5) == -4        # the marker is not below n / m
    assert call(up, 800, 99) == -3 and call(up, 8, 65, M_=0) == -3
    assert call(up, 8, 8, ref=None) == -4
    assert new_id.value == 12345
    assert call(up, NU + 8, NU) == 0 and new_id.value != 12345
    eng.close()
    e.close()


def test_cpp_adapter_warps_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::warp_sample; the result and the info
    equal the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_warp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_warp.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "warped.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n, m = 5 * 512, 3001
    assert "adapter warp ok %d" % m in out, out
    g = np.arange(n, dtype=np.uint64)
    ph = g % 50
    tri = np.where(ph < 25, ph, 50 - ph).astype(np.float32) / np.float32(32.0) - np.float32(0.375)
    x = tri + (((g * 2654435761) & 0xFFFFFFFF) >> 24).astype(np.float32) / np.float32(4096.0)
    want, _, info = M.warp_clip([x.astype(np.float32)], 0, n, m, [(500, 700), (1300, 1301), (2100, 2750)], 256, 96)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == m and first_bad([got], want) is None
    assert ("steps %d searched %d candidates %d max_shift %d segments 4" % (info["steps"], info["searched_steps"], info["candidates"],
                                                                           info["max_shift"])) in out and info["searched_steps"] > 0, out


# ---- 6: beside other work ---------------------------------------------------------------------------------------------------------
def test_a_warp_between_two_renders_leaves_the_master_bit_equal():
    spec = synth.make_session("wrpmix", 3, n_blocks=6, block=128, seed=0x3A93)
    masters = []
    for warp in (False, True):
        eng = build_engine(spec, max_blocks=8)
        up = eng.add_sample("f32", spec.sample_rate, source(2, 3000, seed=7))
        eng.play()
        eng.render(3)
        a, _, _ = eng.ctx.fetch()
        if warp:
            eng.warp_sample(up, 4001, [(700, 1001), (1900, 2502)], 256, 96)
        eng.render(3)
        b, _, _ = eng.ctx.fetch()
        masters.append((bits(np.array(a[:3])).copy(), bits(np.array(b[:3])).copy()))
        eng.close()
    assert np.array_equal(masters[0][0], masters[1][0]) and np.array_equal(masters[0][1], masters[1][1])
    assert masters[0][1].any()


def test_warp_beside_the_audio_thread():
    """The shape of the stretch test (test_gpu_stretch.py): a clip far behind the played range names the big source while the
    threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside one for the
    pin (-3, asked first) — one thread deletes without pause while the other warps until a delete has been refused for the
    pin.  The master is what it is without the calls, and the last result equals the model."""
    NB, FR, WAIT, CALLS = 300, 1 << 19, 60.0, 96
    N, D = 1024, 512
    spec = synth.make_session("wrpthr", 2, n_blocks=NB, block=128, seed=0x3A9712)
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
    m = n * 3 // 2
    mk = [(n // 4, m // 5), (n // 2, m // 2 + 3)]                 # a chain long enough for a delete to land inside the call
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
                results["big"], results["info"] = eng.warp_sample(big, m, mk, N, D, first_frame=first, n_frames=n, channels=2, frames=FR)
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
    print("warp calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    want, _, want_info = M.warp_clip(planes, first, n, m, mk, N, D)
    assert {k: results["info"][k] for k in want_info} == want_info and want_info["searched_steps"] > 100
    assert first_bad(download(eng.ctx, results["big"], 2, m), want) is None
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
