"""wbx_clip_limit and wbx_engine_limit_sample on the device.  Results come back through wbx_clip_download and are compared
BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/limit_model.py, the numpy twin of the header's text; the
limiter's statistics are compared field by field, exactly; |out| <= ceiling is asserted on every result.  Sizes are the
smallest at which the kernels can still go wrong, around their shape constants (T, the frames of a workgroup's tile; P,
the ramp terms of a segment; the band of 2^20 output frames): a lane's 8 frames and the last lane's partial store
(1, 7, 8, 9), one tile less, exactly and more than a frame (T-1, T, T+1), two tiles and a piece (2T+5); ramps of 1, 2, 7
terms (less than one block of 8), of one segment less, exactly and more than a term (P-1, P, P+1) and of two segments and
a piece (2P+3), split several ways between look-ahead, hold and release."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import limit_model as M
import loudness_model as LM
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
T, P, BAND = W.lib().wbx_limit_tile_frames(), W.lib().wbx_limit_segment_terms(), W.lib().wbx_limit_band_frames()
assert (T, P, BAND) == (M.TILE, M.SEGMENT, M.BAND)
FRAMES = [1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 5]
TERMS = [1, 2, 7, P - 1, P, P + 1, 2 * P + 3]
SRC_LEN = 2 * T + 5 + 700
SRC = {1: 1, 2: 2}                                              # channels -> clip id
DST = 100
CEILINGS = [np.float32(1.0), np.float32(0.891251), np.float32(0.5)]
bits = BU.bits


def source(channels, n=SRC_LEN, seed=0x11417, every=97):
    """noise of +-0.5 around a small offset, every `every`-th sample (the channels at different places) four times as
    large: with the ceilings used here most frames pass and a few are limited"""
    rng = np.random.default_rng(seed + channels)
    planes = [(rng.uniform(-0.5, 0.5, n) + 0.0625 * (1 - 2 * k)).astype(np.float32) for k in range(channels)]
    for k, p in enumerate(planes):
        p[11 * k + 3::every] *= np.float32(4.0)
    return planes


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


def limit_and_check(c, clip, planes, first, n, ceiling, drive, A, H, R, dst=DST, where=None):
    """one call against the model: every output bit, the guarantee, wbx_limit_stats and stats_of_result.  Returns (the
    result's planes, the limiter's statistics)"""
    ch = len(planes)
    want, want_ls = M.limit_clip(planes, first, n, ceiling, drive, A, H, R)
    ls, st = c.clip_limit(clip, dst, first, n, ceiling, drive, A, H, R, stats_channels=ch)
    got = download(c, dst, ch, n)
    where = where or (ch, first, n, float(ceiling), drive, A, H, R)
    assert first_bad(got, want) is None, (where, first_bad(got, want))
    assert all(np.all(np.abs(g) <= np.float32(ceiling)) for g in got), where
    assert ls == want_ls, (where, ls, want_ls)
    check_stats(st, FX.measure(want), n, where)
    return got, ls


# ---- 1: lengths x ramp lengths, mono and stereo, several splits of the ramp ----------------------------------------------------
def split(K, i):
    """the i-th way to cut K terms into look-ahead, hold and release"""
    way = i % 4
    if way == 0:
        return 0, 0, K
    if way == 1:
        A = min(K - 1, M.MAX_LOOKAHEAD)
        return A, 0, K - A
    if way == 2:
        A = min(K // 3, M.MAX_LOOKAHEAD)
        H = (K - A) // 2
        return A, H, K - A - H
    return 0, K - 1, 1


def shape_of_call(n, K, i):
    """the i-th variation of a case: the split, the range's start (inside the clip; on odd i the range ENDS on the clip's
    last frame), the ceiling and the drive"""
    A, H, R = split(K, i)
    first = SRC_LEN - n if i % 2 else (5, 0, 64)[i % 3]
    assert A + H + R == K and R >= 1 and first >= 0 and first + n <= SRC_LEN
    return A, H, R, first, CEILINGS[i % 3], (1.0, 1.5, -0.75)[(i // 2) % 3]


CASES = [(n, K, ni + ki) for ni, n in enumerate(FRAMES) for ki, K in enumerate(TERMS)]


def test_the_matrix_covers_what_it_claims():
    shapes = [shape_of_call(n, K, i + ch) for n, K, i in CASES for ch in (1, 2)]
    looks, holds, releases = ({s[k] for s in shapes} for k in range(3))
    assert {0, 1, P // 3, P - 1, 4096} <= looks and {0, 1, P - 1, P} <= holds and {1, 2, 3, 7, P, 2 * P + 3} <= releases
    assert len({float(s[4]) for s in shapes}) == 3 and {s[5] for s in shapes} == {1.0, 1.5, -0.75}
    assert {(ch, s[3] + n == SRC_LEN) for n, K, i in CASES for ch in (1, 2) for s in [shape_of_call(n, K, i + ch)]} == {
        (1, True), (1, False), (2, True), (2, False)}          # both channel counts with ranges that end on the clip's last frame
    assert any(0 < s[3] and s[3] + n < SRC_LEN for n, K, i in CASES for s in [shape_of_call(n, K, i + 1)])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "frames%d-terms%d" % (c[0], c[1]))
def test_limit_matrix(ctx, case):
    n, K, i = case
    for ch in (1, 2):
        A, H, R, first, ceiling, drive = shape_of_call(n, K, i + ch)
        limit_and_check(ctx, SRC[ch], ctx.src[ch], first, n, ceiling, drive, A, H, R)


# ---- 2: where the peaks stand ------------------------------------------------------------------------------------------------------
def quiet_with_peaks(n, at, channels=1, seed=0x9EA5):
    rng = np.random.default_rng(seed)
    planes = [rng.uniform(-0.2, 0.2, n).astype(np.float32) for _ in range(channels)]
    for j, f in enumerate(at):
        planes[j % channels][f] = np.float32((2.0, -3.0, 1.25)[j % 3])
    return planes


@pytest.mark.parametrize("channels", [1, 2])
def test_peaks_on_the_ends_on_tile_seams_and_with_a_release_across_a_segment_seam(ctx, channels):
    """peaks on frame 0 and on the last frame, on both sides of both tile seams; the ramp has 16 + 100 + 3000 terms, so every
    peak's release runs from one segment of the walk into the next"""
    n = 2 * T + 100
    planes = quiet_with_peaks(n, [0, n - 1, T - 1, T, 2 * T - 1, 2 * T], channels)
    ctx.clip_upload(50, "f32", RATE, planes)
    _, ls = limit_and_check(ctx, 50, planes, 0, n, np.float32(0.5), 1.0, 16, 100, 3000)
    assert ls["limited_frames"] > T and ls["peak_in"] == 3.0 and 0.0 <= 0.5 / 3.0 - ls["min_gain"] < 1e-15
    for A, H, R in ((0, 0, 1), (4096, 0, 1), (1, P - 2, 1), (7, 0, P + 9)):
        limit_and_check(ctx, 50, planes, 0, n, np.float32(0.5), 1.0, A, H, R)
    # peaks in curve frames the look-ahead adds: the range starts right behind one and ends right before another
    limit_and_check(ctx, 50, planes, 1, n - 2, np.float32(0.5), 1.0, 16, 100, 3000)


@pytest.mark.parametrize("channels", [1, 2])
def test_a_source_that_is_silent_but_for_one_peak_alternates_skipped_and_walked_segments(ctx, channels):
    """three tiles, a ramp of 2P + 3 terms and ONE sample above the ceiling: of the segments a tile walks only those whose
    staged span holds the peak can lower anything; the others are skipped by the vote"""
    n, K = 3 * T + 11, 2 * P + 3
    for at in (T + 5, 0, n - 1):
        planes = quiet_with_peaks(n, [at], channels, seed=at)
        ctx.clip_upload(51, "f32", RATE, planes)
        for i in range(3):
            A, H, R = split(K, i)
            _, ls = limit_and_check(ctx, 51, planes, 0, n, np.float32(0.25), 1.0, A, H, R)
            assert ls["min_gain_frame"] == at and ls["min_gain"] == 0.125 and 0 < ls["limited_frames"] <= K + A   # (the curve is below 1.0 on at most K frames, the average of A + 1 of them on A more)


def test_a_peak_on_the_band_seam():
    """2^20 + 2053 frames, mono: two bands.  Peaks on both sides of the seam, a short ramp: the second band recomputes the
    A curve frames in front of it, and the statistics of the two bands are merged"""
    c = W.MixContext(4, block=128)
    n = BAND + 2053
    planes = quiet_with_peaks(n, [BAND - 1, BAND, 17, BAND + 2040, BAND - 9], 1, seed=0xBA4D)   # (-3.0 on BAND - 9 and on BAND)
    c.clip_upload(1, "f32", RATE, planes)
    _, ls = limit_and_check(c, 1, planes, 0, n, np.float32(0.5), 1.0, 8, 3, 40, dst=2)
    assert ls["min_gain_frame"] == BAND - 9 and ls["limited_frames"] > 100   # the same gain in both bands: the first frame wins
    c.close()


# ---- 3: pass-through, edge inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_a_clip_under_the_ceiling_comes_back_bit_for_bit(ctx, channels):
    n = 2 * T + 5
    rng = np.random.default_rng(0x9A55 + channels)
    planes = [rng.uniform(-0.89, 0.89, n).astype(np.float32) for _ in range(channels)]
    planes[0][:4] = -0.0, 0.891251, -0.891251, 1e-42            # a signed zero, the ceiling itself, a denormal
    ctx.clip_upload(52, "f32", RATE, planes)
    for A, H, R in ((72, 0, 4800), (0, 0, 1), (4096, 9, 7)):
        got, ls = limit_and_check(ctx, 52, planes, 0, n, np.float32(0.891251), 1.0, A, H, R)
        assert first_bad(got, planes) is None
        assert ls["limited_frames"] == 0 and ls["min_gain"] == 1.0 and ls["min_gain_frame"] == 0


@pytest.mark.parametrize("channels", [1, 2])
def test_values_that_are_not_finite_enter_as_zero(ctx, channels):
    n = T + 600
    planes = source(channels, n, seed=0x0FF)
    zeroed = [p.copy() for p in planes]
    for c, (p, z) in enumerate(zip(planes, zeroed)):
        at = np.array([0, 5, 300, T - 1, T, T + 1, n - 1]) - c * np.array([0, 1, 1, 1, 1, 1, 1])
        p[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
        z[at] = 0.0
    planes[0].view(np.uint32)[40] = 0xFFC12345                  # a NaN with a payload and a sign
    zeroed[0][40] = 0.0
    ctx.clip_upload(53, "f32", RATE, planes)
    for drive in (1.0, -2.0):
        want, _ = M.limit_clip(planes, 0, n, np.float32(0.5), drive, 20, 5, 300)
        assert first_bad(want, M.limit_clip(zeroed, 0, n, np.float32(0.5), drive, 20, 5, 300)[0]) is None
        assert np.all(np.isfinite(np.stack(want)))
        limit_and_check(ctx, 53, planes, 0, n, np.float32(0.5), drive, 20, 5, 300)


@pytest.mark.parametrize("channels", [1, 2])
def test_frames_beside_the_range_do_not_count(ctx, channels):
    """loud samples and NaNs in front of and behind the range: the result is that of the quiet range alone"""
    planes = source(channels, 3000, seed=0xBE51DE)
    for p in planes:
        p[:200], p[190:200], p[2700:], p[2710:2720] = 1e30, np.nan, -1e30, np.nan
    ctx.clip_upload(54, "f32", RATE, planes)
    for first, n in ((200, 2500), (200, 1), (2699, 1), (200, 9)):
        alone = [p[first:first + n].copy() for p in planes]
        want, want_ls = M.limit_clip(alone, 0, n, np.float32(0.5), 1.0, 64, 10, 500)
        got, ls = limit_and_check(ctx, 54, planes, first, n, np.float32(0.5), 1.0, 64, 10, 500)
        assert first_bad(got, want) is None and ls == want_ls and ls["peak_in"] < 4.0


@pytest.mark.parametrize("ceiling", [np.float32(1.0), np.float32(0.891251), np.float32(M.FLT_MIN)], ids=["1", "-1dB", "FLT_MIN"])
def test_huge_samples_drives_and_ceilings(ctx, ceiling):
    """samples of 3e38 with a drive of 2^32 (d reaches 1.3e48), a negative drive, drives below 1, down to the smallest
    ceiling: the gain falls to 1e-86 and the guarantee holds"""
    n = T + 77
    planes = source(2, n, seed=0xB16)
    planes[0][[0, 9, T, n - 1]] = 3e38, -3e38, 3e38, -3e38
    planes[1][[1, T - 1]] = -3e38, 1e-40
    ctx.clip_upload(55, "f32", RATE, planes)
    for drive in (2.0 ** 32, -2.0 ** 32, -1.0, 0.125, -2.0 ** -40):
        _, ls = limit_and_check(ctx, 55, planes, 0, n, ceiling, drive, 30, 4, 700)
        assert ls["peak_in"] == abs(drive) * float(np.float32(3e38))
        need = float(np.float64(ceiling) / np.float64(ls["peak_in"]))   # (the average of A + 1 such values may round below it)
        assert need * (1.0 - 1e-14) <= ls["min_gain"] <= need and ls["min_gain_frame"] in (0, 1, 9)
    ctx.clip_upload(56, "f32", RATE, planes[:1])
    limit_and_check(ctx, 56, planes[:1], 3, n - 3, ceiling, -2.0 ** 32, 0, 0, 1)


def test_time_of_the_last_limit():
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_limit_ms(c.h, C.byref(out)) == -4 and out.value == 7.0        # none yet
    c.clip_upload(1, "f32", RATE, source(1, 5000))
    assert c.L.wbx_limit_ms(c.h, None) == -4
    c.clip_limit(1, 3, 0, 5000, 0.5)
    assert 0.0 < c.limit_ms() < 1000.0
    c.close()


# ---- 4: the pool -------------------------------------------------------------------------------------------------------------------
def test_a_replaced_dst_takes_the_old_extents_place_and_a_delete_restores_the_pool():
    c = W.MixContext(4, block=128)
    planes = source(2, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(2, "f32", RATE, [np.ones(4000, dtype=np.float32)] * 2)        # a neighbour behind what comes next
    base = c.pool_stats()
    c.clip_limit(1, 10, 0, 4000, 0.5)
    with_one = c.pool_stats()
    assert with_one[0] == base[0] and with_one[1] == base[1] and with_one[2] > base[2]
    for first in (5, 900):                                      # replaced by results of the same length: the same figures
        limit_and_check(c, 1, planes, first, 4000, np.float32(0.5), 1.0, 72, 0, 4800, dst=10)
        assert c.pool_stats() == with_one
    limit_and_check(c, 1, planes, 0, 700, np.float32(0.5), 1.0, 0, 0, 1, dst=10)   # ... by a shorter one: nothing more is reserved or live
    assert c.pool_stats()[:2] == with_one[:2] and c.pool_stats()[2] <= with_one[2]
    assert all(np.all(p == 1.0) for p in download(c, 2, 2, 4000))
    assert c.L.wbx_clip_free(c.h, 10) == 0
    assert c.pool_stats() == base
    c.close()


def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    ctx.clip_limit(SRC[2], DST, 0, 64, 0.5, 1.0, 8, 0, 48)
    kept = bits(np.stack(download(ctx, DST, 2, 64))).tolist()
    ctx.clip_upload(60, "i16", RATE, [np.arange(64, dtype=np.int16)] * 2)
    ls, st = _ffi.LimitStats(), _ffi.ClipStats()
    S = SRC[2]

    def refused(status, why, src=S, dst=DST, first=0, n=64, ceiling=0.5, drive=1.0, A=8, H=0, R=48):
        before = ctx.pool_stats()
        ls.limited_frames = 777
        got = L.wbx_clip_limit(ctx.h, src, dst, first, n, ceiling, drive, A, H, R, C.byref(ls), C.byref(st))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 64))).tolist() == kept and ls.limited_frames == 777

    refused(-4, b"unknown source", src=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"past the clip", first=SRC_LEN - 10, n=11)
    refused(-4, b"past the clip", first=SRC_LEN + 1, n=1)
    refused(-4, b"past the clip", first=(1 << 64) - 1, n=2)     # a sum that wraps
    refused(-4, b"may not replace", dst=S)
    for v in (0.0, -0.5, np.nan, np.inf, M.FLT_MIN / 2):
        refused(-4, b"ceiling", ceiling=v)
    for v in (0.0, -0.0, np.nan, np.inf, -np.inf, 2.0 ** 33, -2.0 ** 32 * (1 + 2.0 ** -52)):
        refused(-4, b"drive", drive=v)
    refused(-4, b"lookahead", A=4097)
    refused(-4, b"hold", H=65537)
    refused(-4, b"release", R=0)
    refused(-4, b"release", R=(1 << 20) + 1)
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16)                 # judged on the arithmetic: no clip is that long
    refused(-3, b"not F32", src=60)                             # (a clip of more than 2 channels cannot exist in the pool)
    refused(-3, b"2^44", n=(1 << 24) + 1, A=0, H=0, R=1 << 20)
    refused(-4, b"past the clip", n=1 << 24, A=0, H=0, R=1 << 20)               # ... at the cap the sizes pass, the clip does not
    refused(-3, b"2^44", src=60, n=1 << 30, A=4096, H=65536, R=1 << 20)          # the sizes are judged before the clip is looked at
    refused(-4, b"ceiling", src=60, ceiling=0.0)
    # what is not refused: the limits themselves
    ctx.clip_limit(S, 62, SRC_LEN - 1, 1, M.FLT_MIN, 2.0 ** 32, 4096, 65536, 1 << 20)
    ctx.clip_limit(S, 62, 0, 9, 3e38, -2.0 ** 32, 0, 0, 1)
    assert L.wbx_clip_free(ctx.h, 62) == 0


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 20
    planes = source(2, n)
    c.clip_upload(1, "f32", RATE, planes)                       # 8 MiB in the first slab (64 MiB)
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_limit(1, 10 + len(made), 0, n, 0.5, 1.0, 4, 0, 12)           # 8 MiB each
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            assert c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    want, _ = M.limit_clip([p[:4096] for p in planes], 0, 4096, np.float32(0.5), 1.0, 4, 0, 12)
    got = [c.clip_download(made[-1], k, n, np.float32)[:4000] for k in range(2)]
    assert first_bad(got, [w[:4000] for w in want]) is None      # (the model saw 4096 frames: the look-ahead of the last 4 differs)
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.pool_limit(0)
    c.close()


# ---- 5: through the engine -----------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_limit_sample_of_an_upload_a_take_a_bounce_and_an_earlier_result():
    spec = synth.make_session("limit2", 3, n_blocks=6, block=128, seed=0x11412)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
    # a bounce of track 1, pre-fader
    lo, hi = BU.bounce_range(spec, 5)
    ids, nb = eng.bounce(lo, hi, [("track", 1, "pre")])
    stem = [np.ascontiguousarray(p) for p in eng.bounce_download(ids[0], nb)]
    assert np.any(np.stack(stem) != 0.0)
    # a take on track 0
    eng.set_audio_channel_config(2, spec.channels, spec.block, rate)
    eng.set_track_input(0, "external_mono", 0, True)
    x = source(1, 5 * spec.block, seed=0x7A4E, every=41)[0]
    inp, out = W.AudioBuffer(spec.block, 2), W.AudioBuffer(spec.block, spec.channels)
    eng.record()
    for b in range(5):
        inp.channel_buffers[0][:] = x[b * spec.block:(b + 1) * spec.block]
        inp.channel_buffers[1][:] = 0.0
        eng.process(inp, out, float(rate))
    frames = eng.record_info(0)["frames"]
    eng.stop_record()
    eng.stop()
    eng.set_playhead_position(0.0)
    take = max(c[5] for c in eng.clips(eng.tracks[0]))
    assert frames == len(x) and first_bad(download(eng.ctx, take, 1, frames), [x]) is None
    # an upload
    NU = 3 * LM.hop_frames(rate)                                # three hops of the loudness meter
    planes = source(2, NU + 8, seed=0x0B)
    up = eng.add_sample("f32", rate, planes)

    # the upload, by times and decibels: the Python conversions, then the model on what they gave
    A, H, R = W.limit_frames(rate, 1.5, 2.0, 50.0)
    ceiling, drive = np.float32(10.0 ** (-1.0 / 20.0)), 10.0 ** (3.0 / 20.0)
    c_up, ls, st = eng.limit_sample(up, ceiling_db=-1.0, lookahead_ms=1.5, hold_ms=2.0, release_ms=50.0, drive_db=3.0, first_frame=4,
                                    n_frames=NU, stats=True)
    want_up, want_ls = M.limit_clip(planes, 4, NU, ceiling, drive, A, H, R)
    assert eng._sample_shape[c_up] == (NU, 2) and ls == want_ls and ls["limited_frames"] > 0
    assert first_bad(download(eng.ctx, c_up, 2, NU), want_up) is None
    assert all(np.all(np.abs(w) <= ceiling) for w in want_up)
    check_stats(st, FX.measure(want_up), NU, "limit_sample's stats")
    # the mono take, in frames
    c_take, ls = eng.limit_sample(take, ceiling_db=-6.0, shape=(16, 0, 200), frames=frames, channels=1)
    want_take, want_ls = M.limit_clip([x], 0, frames, np.float32(10.0 ** (-6.0 / 20.0)), 1.0, 16, 0, 200)
    assert eng._sample_shape[c_take] == (frames, 1) and ls == want_ls
    assert first_bad(download(eng.ctx, c_take, 1, frames), want_take) is None
    # the bounce, a range of it, driven hard
    c_stem, ls = eng.limit_sample(ids[0], ceiling_db=-20.0, drive_db=12.0, shape=(8, 4, 100), first_frame=7, n_frames=nb - 9)
    want_stem, want_ls = M.limit_clip(stem, 7, nb - 9, np.float32(10.0 ** (-20.0 / 20.0)), 10.0 ** (12.0 / 20.0), 8, 4, 100)
    assert ls == want_ls and first_bad(download(eng.ctx, c_stem, spec.channels, nb - 9), want_stem) is None
    # of an earlier result: limited again under a lower ceiling
    again, ls = eng.limit_sample(c_up, ceiling_db=-12.0, shape=(0, 0, 1), n_frames=600)
    want_again, want_ls = M.limit_clip(want_up, 0, 600, np.float32(10.0 ** (-12.0 / 20.0)), 1.0, 0, 0, 1)
    assert ls == want_ls and first_bad(download(eng.ctx, again, 2, 600), want_again) is None

    # the limited upload on a track, against the oracle playing the MODEL's clip
    unit = BU.block_beats(spec.block, rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    for t in range(3):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
        while e.clips(t):
            e.delete_clip(t, 0)
    eng.add_audio_clip(eng.tracks[2], "limited", 0.5 * unit, 5.5 * unit, 0.0, c_up, 1.0, 1.0)
    assert e.add_audio_clip(2, 0.5 * unit, 5.5 * unit, 0.0, oracle_sample(e, want_up, rate), 1.0, 1.0) == 0
    e.play()
    eng.play()
    eng.render(6)
    m, _, _ = eng.ctx.fetch()
    heard = False
    for b in range(6):
        om, _ = e.process()
        assert np.array_equal(bits(m[b]), bits(om)), b
        heard = heard or bool(om.any())
    assert heard
    # exported, and loudness-measured: an ordinary sample
    got, _ = eng.export_sample(c_up, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(want_up, axis=1).reshape(-1).view(np.uint32))
    _, E = eng.loudness_sample(c_up, energies=True, rate=rate)
    want_E = LM.hop_energies(want_up, 0, NU, rate)
    assert E.shape == want_E.shape == (2, 3) and np.array_equal(E.view(np.uint64), want_E.view(np.uint64))
    with pytest.raises(W.WbxError):
        eng.delete_sample(c_up)                                 # a clip names it
    eng.delete_sample(again)
    # refusals create no sample
    L, new = W.lib(), C.c_uint32(12345)
    before = eng.ctx.pool_stats()
    call = lambda s, n, ceiling=0.5, drive=1.0, A=8, H=0, R=48, ref=C.byref(new): L.wbx_engine_limit_sample(
        eng.h, s, 0, n, ceiling, drive, A, H, R, ref, None, None)
    assert call(9999, 8) == -4
    assert call(again, 8) == -4                                 # deleted
    assert call(up, NU + 9) == -4
    assert call(up, 0) == -4
    assert call(up, 8, ceiling=0.0) == -4
    assert call(up, 8, drive=np.nan) == -4
    assert call(up, 8, A=4097) == -4
    assert call(up, 8, R=0) == -4
    assert call(up, 8, ref=None) == -4
    assert call(up, (1 << 24) + 1, A=0, R=1 << 20) == -3
    assert new.value == 12345 and eng.ctx.pool_stats() == before
    eng.close()
    e.close()


def test_maximize_sample_reaches_for_a_target_under_the_ceiling():
    """one second of quiet stereo noise with a tall burst every 50 ms, taken to -14 LUFS under -1 dBFS in one pass: no
    sample above the ceiling, the loudness at or under the target — under it by what the limiter took from the bursts"""
    spec = synth.make_session("limit3", 1, n_blocks=2, block=128, seed=0x11413)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=2)
    n = rate
    rng = np.random.default_rng(0x3A51)
    planes = [rng.uniform(-0.02, 0.02, n).astype(np.float32) for _ in range(2)]
    for p in planes:
        for at in range(100, n - 40, rate // 20):
            p[at:at + 24] *= np.float32(12.0)
    s = eng.add_sample("f32", rate, planes)
    before = eng.loudness_sample(s)
    new, info = eng.maximize_sample(s, -14.0, ceiling_db=-1.0)
    ceiling = np.float32(10.0 ** (-1.0 / 20.0))
    got = download(eng.ctx, new, 2, n)
    A, H, R = W.limit_frames(rate)
    want, want_ls = M.limit_clip(planes, 0, n, ceiling, 10.0 ** ((-14.0 - before["integrated"]) / 20.0), A, H, R)
    assert first_bad(got, want) is None and info["limit"] == want_ls
    assert max(float(np.max(np.abs(g))) for g in got) <= ceiling
    assert info["limit"]["limited_frames"] > 0 and info["drive_db"] == -14.0 - before["integrated"] and info["drive_db"] > 6.0
    print("maximize: before %.3f LUFS, drive %.3f dB, after %.3f LUFS, true peak %s" % (before["integrated"], info["drive_db"],
                                                                                       info["loudness"], info["true_peak"]))
    assert info["loudness"] <= -14.0 and info["loudness"] > -20.0
    assert info["loudness"] == eng.loudness_sample(new)["integrated"]
    assert len(info["true_peak"]) == 2 and all(0.0 < t < 2.0 for t in info["true_peak"])
    eng.close()


def test_cpp_adapter_limits_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::limit_sample with a drive of 3 under
    -1 dBFS; the result and the statistics equal the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_limit")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_limit.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "limited.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n = 5 * 512
    assert "adapter limit ok %d" % n in out, out
    idx = np.arange(n, dtype=np.uint64)
    x = (((idx * 2654435761) & 0xFFFFFFFF) & 0xFFFF).astype(np.float32) / np.float32(65536.0) - np.float32(0.25)
    want, ls = M.limit_clip([x], 0, n, np.float32(0.891251), 3.0, 72, 10, 480)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == n and first_bad([got], want) is None and np.all(np.abs(got) <= np.float32(0.891251))
    assert ("peak %.9g limited %d min_gain %.17g at %d peak_in %.17g" % (np.max(np.abs(want[0])), ls["limited_frames"], ls["min_gain"],
                                                                        ls["min_gain_frame"], ls["peak_in"])) in out, out


# ---- 6: beside the audio thread -------------------------------------------------------------------------------------------------
def test_limits_beside_the_audio_thread():
    """The shape of the convolution's test (test_gpu_convolve.py): a clip far behind the played range names the big sample
    while the threads run, so a delete of it can never succeed — between two limits it is refused for the clip (-4), inside
    one for the pin (-3, asked first) — one thread deletes without pause while the other limits until a delete has been
    refused for the pin.  The source is loud everywhere, so every segment of the 2^14-term ramp is walked.  The master is
    what it is without the limits, and the last result equals the model where it is compared: the first, a middle and the
    last tile."""
    NB, FR, WAIT, CALLS = 300, 1 << 20, 60.0, 64
    A, H, R = 64, 0, (1 << 14) - 64
    spec = synth.make_session("limthr", 2, n_blocks=NB, block=128, seed=0x114712)
    rng = np.random.default_rng(37)
    planes = [rng.uniform(-2.0, 2.0, FR).astype(np.float32) for _ in range(2)]

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
            key = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key] = seen.get(key, 0) + 1
            if st == -3:
                refused.set()

    def editor():
        try:
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["big"], results["ls"] = eng.limit_sample(big, ceiling_db=-6.0, shape=(A, H, R), first_frame=first, n_frames=n,
                                                                 channels=2, frames=FR)
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
    print("limit calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in m for _, m in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every limit read a live clip: the result is the model's, bit for bit.  A window's gains depend on A frames after it
    # and on H + R frames before it: the model gets those and the comparison is made on the tile in the middle
    ceiling = np.float32(10.0 ** (-6.0 / 20.0))
    assert results["ls"]["limited_frames"] > n // 2
    for at in (0, (n // 2 // T) * T - 9, n - T - 3):
        lo, hi = max(0, at - H - R - A), min(n, at + T + 3 + A)
        want, _ = M.limit_clip(planes, first + lo, hi - lo, ceiling, 1.0, A, H, R)
        got = [eng.ctx.clip_download(results["big"], k, n, np.float32)[at:at + T + 3] for k in range(2)]
        assert first_bad(got, [w[at - lo:at - lo + T + 3] for w in want]) is None, at
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    new = C.c_uint32(12345)
    assert L.wbx_engine_limit_sample(eng.h, big, 0, 8, 0.5, 1.0, 8, 0, 48, C.byref(new), None, None) == -4 and new.value == 12345
    eng.close()
