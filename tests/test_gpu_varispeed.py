"""wbx_clip_varispeed and wbx_engine_varispeed_sample on the device.  Results come back through wbx_clip_download (or
wbx_clip_export for windows of a long result) and are compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with
tests/varispeed_model.py, the numpy twin of the header's text; stats_of_result against tests/clipfx_model.py's measure.
Sizes are the smallest at which the kernel can still go wrong: a lane's 4 frames and the last lane's partial store (1, 15,
17), one interval, a tile of 1024 less, exactly and more than a frame, four tiles and a piece, tiles of 1, 2 and 64
intervals next to each other, every quality's phase shift, and one run of 2^16 + 3 tiles for the capped grid's second pass."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import clipfx_model as FX
import second_pass as SP
import varispeed_model as M
import warp_model as WM
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 6000
SRC = {1: 1, 2: 2}                                              # channels -> clip id
DST = 100
ONE = 1 << 32
QUALITIES = [M.FAST, M.GOOD, M.BEST]
SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 4 * 1024 + 3]
_TABS = {}


def tabs(q, guard=(1, 1)):
    """the model's tables, built once per (quality, guard) and never changed"""
    key = (q,) + tuple(guard)
    if key not in _TABS:
        _TABS[key] = M.tables(q, *guard)
    return _TABS[key]


def source(channels, n=SRC_LEN, seed=0x7A9):
    rng = np.random.default_rng(seed + channels)
    return [rng.uniform(-1.0, 1.0, n).astype(np.float32) for _ in range(channels)]


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
    assert FX.exact_fields_equal(got, want), (where, got, {k: want[k] for k in FX.EXACT})
    for k, mag in (("sum", "abs_sum"), ("sum_sq", "abs_sum_sq")):
        for g, w, a in zip(got[k], want[k], want[mag]):
            if np.isfinite(a):
                assert abs(g - w) <= n * 2.0 ** -52 * a, (where, k, g, w)


def run_and_check(c, clip, planes, first, n, out, knots, g, q, guard=(1, 1), dst=DST):
    """one call against the model: the model's check accepts it, every output bit, stats_of_result"""
    ch = len(planes)
    assert M.check(knots, len(knots), g, n, out, q, *guard) == (0, ""), M.check(knots, len(knots), g, n, out, q, *guard)
    want = M.varispeed(planes, first, n, out, knots, g, q, *guard, tabs=tabs(q, guard))
    st = c.clip_varispeed(clip, dst, first, n, out, knots, g, q, guard[0], guard[1], stats_channels=ch)
    got = download(c, dst, ch, out)
    where = (ch, first, n, out, g, q, guard)
    assert first_bad(got, want) is None, (where, first_bad(got, want))
    check_stats(st, FX.measure(want), out, where)
    return got


# ---- 1: smallest shapes and tile seams ---------------------------------------------------------------------------------------
def curve(name, out, q):
    """(knots, guard) of `out` output frames at knot_shift 4; positions stay within [-2^16, SRC_LEN - 3 + 2^16] frames"""
    K = M.n_knots(out, 4)
    i = np.arange(K, dtype=object)
    if name == "speed 1":
        kn = [int(v) * 16 * ONE for v in i]
    elif name == "irrational":
        s = int(0.7390851332151607 * ONE)
        kn = [int(3.25 * ONE) + int(v) * 16 * s for v in i]
    elif name == "last fraction":                                # fr = 0xFFFFFFFF at every output: p = P - 1, the largest t
        kn = [((10 + int(v) * 16) << 32) + 0xFFFFFFFF for v in i]
    elif name == "speed 0":
        kn = [(777 << 32) + 0x80001234] * K
    elif name == "descending":                                   # a difference 16 does not divide: the shift floors
        s = int(0.9137 * ONE) | 1
        kn = [(5000 << 32) - int(v) * (16 * s + 5) for v in i]
    elif name == "scratch":                                      # forward, back, forward
        kn = [int(round((1500 + 0.3 * 16 * int(v) + 400.0 * np.sin(2 * np.pi * 16 * int(v) / 700.0)) * ONE)) for v in i]
        return np.array(kn, dtype=np.int64), (4, 1)
    elif name == "tiles 1 2 64":
        Lm = M.SPAN_MAX - M.plan(q)["T"]                         # the widest run of knot frames a tile holds
        head = [0, Lm - 100, Lm + 50, Lm - 1950, -50]
        kn = [(head[int(v)] if v < 5 else -50 + 16 * (int(v) - 4)) * ONE + 12345 * int(v) for v in i]
    else:
        raise KeyError(name)
    return np.array(kn, dtype=np.int64), (1, 1)


CURVES = ["speed 1", "irrational", "last fraction", "speed 0", "descending", "scratch", "tiles 1 2 64"]


@pytest.mark.parametrize("q", QUALITIES, ids=["fast", "good", "best"])
@pytest.mark.parametrize("name", CURVES)
def test_smallest_shapes_and_tile_seams(ctx, name, q):
    assert M.plan(q)["s"] == {M.FAST: 24, M.GOOD: 23, M.BEST: 21}[q]
    for ch in (1, 2):
        for k, out in enumerate(SIZES):
            kn, guard = curve(name, out, q)
            first = (0, 3)[(k + ch) % 2]
            run_and_check(ctx, SRC[ch], ctx.src[ch], first, SRC_LEN - first, out, kn, 4, q, guard)
    kn, guard = curve(name, SIZES[-1], q)
    t = W.varispeed_tiles(kn, 4, SRC_LEN, SIZES[-1], q, *guard)
    assert t == M.tiles(kn, SIZES[-1], 4, M.plan(q, *guard))
    if name == "tiles 1 2 64":
        assert [r[1] for r in t[:4]] == [16, 32, 1024, 1024], t[:5]
    if name == "last fraction":
        pos = M.positions(kn, 4, 0, SIZES[-1])
        assert np.all(pos & 0xFFFFFFFF == 0xFFFFFFFF)


# ---- 2: composition on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", QUALITIES, ids=["fast", "good", "best"])
@pytest.mark.parametrize("src,dst,guard", [(1, 2, (1, 1)), (1, 4, (1, 1)), (2, 1, (2, 1)), (3, 2, (3, 2))], ids=lambda v: str(v))
def test_a_constant_speed_on_table_rows_is_the_conversion_on_the_device(ctx, src, dst, guard, q):
    """t = 0 on these curves, so y = (float)A: the conversion's chain over the conversion's rows"""
    first, n, ch = 9, 3000, 2
    rate = RATE * dst // src
    out = W.resample_frames(RATE, rate, n)
    ctx.clip_resample(SRC[ch], 110, first, n, rate, q)
    kn = M.constant_knots(out, 4, src, dst)
    ctx.clip_varispeed(SRC[ch], 111, first, n, out, kn, 4, q, *guard)
    assert first_bad(download(ctx, 111, ch, out), download(ctx, 110, ch, out)) is None
    for k in (110, 111):
        assert ctx.L.wbx_clip_free(ctx.h, k) == 0


# ---- 3: the edges of the range ----------------------------------------------------------------------------------------------------
def test_from_frame_0_to_the_last_frame_and_far_outside(ctx):
    for ch in (1, 2):
        kn = M.constant_knots(SRC_LEN, 6, 1, 1)                     # the whole clip at speed 1: taps before frame 0, past the last
        run_and_check(ctx, SRC[ch], ctx.src[ch], 0, SRC_LEN, SRC_LEN, kn, 6, M.GOOD)
        # from -2^16 frames to n + 2^16: zeros come in at both ends, 3808 frames per interval of 1024 outputs
        out, g = 36 * 1024, 10
        a, b = -(M.MARGIN << 32), (SRC_LEN + M.MARGIN) << 32
        kn = np.array([a + (b - a) * i // 36 for i in range(37)], dtype=np.int64)
        got = run_and_check(ctx, SRC[ch], ctx.src[ch], 0, SRC_LEN, out, kn, g, M.GOOD)
        assert all(np.all(p[:16 * 1024] == 0.0) and np.all(p[-16 * 1024:] == 0.0) and np.any(p != 0.0) for p in got)
        assert all(np.all(p[:16 * 1024].view(np.uint32) == 0) for p in got)     # +0.0: the staged zero is the masked tap


def test_nothing_beside_the_range_is_read():
    """a range between neighbours of +-3e38 — the first clip of a fresh context's first slab —: the same bits as the range
    alone, although the curve starts before the range and runs past it"""
    c = W.MixContext(4, block=128)
    for ch in (1, 2):
        inner = source(ch, 1500, seed=0x33)
        walled = [np.concatenate([np.full(200, 3e38 * (1 - 2 * (k & 1)), np.float32), p, np.full(200, -3e38, np.float32)]) for k, p in enumerate(inner)]
        c.clip_upload(1, "f32", RATE, walled)
        out = 2051
        j = np.arange(M.n_knots(out, 4)) * 16.0
        kn = np.array([int(round((-90.0 + 0.85 * v + 60.0 * np.sin(v / 50.0)) * ONE)) for v in j], dtype=np.int64)
        assert kn.min() < -50 * ONE and kn.max() > 1550 * ONE
        for q in QUALITIES:
            got = run_and_check(c, 1, walled, 200, 1500, out, kn, 4, q)
            assert first_bad(got, M.varispeed(inner, 0, 1500, out, kn, 4, q, tabs=tabs(q))) is None
            assert all(np.all(np.abs(p) < 10.0) for p in got)
        # the range at frame 0 of the slab's first clip: what lies before the slab is never touched
        c.clip_upload(1, "f32", RATE, inner)
        run_and_check(c, 1, inner, 0, 1500, out, kn, 4, M.BEST)
    c.close()


@pytest.mark.parametrize("q", QUALITIES, ids=["fast", "good", "best"])
def test_values_that_are_not_finite_and_overflow(q):
    c = W.MixContext(4, block=128)
    n, out = 1300, 1500
    for ch in (1, 2):
        planes = source(ch, n, seed=0x44)
        p = planes[0]
        p[100], p[400], p[401], p[700] = np.nan, np.inf, -np.inf, -0.0
        p[900:960] = np.float32(3e38) * np.where(np.arange(60) % 2, np.float32(-1.0), np.float32(1.0))   # the sum overflows fp32
        p[1000:1010] = np.float32(3e38)
        p[1100:1200] = np.float32(-0.0)
        c.clip_upload(1, "f32", RATE, planes)
        kn = np.array([int(i * 16 * 0.8613 * ONE) for i in range(M.n_knots(out, 4))], dtype=np.int64)
        got = run_and_check(c, 1, planes, 0, n, out, kn, 4, q)
        bits = got[0].view(np.uint32)
        assert np.isnan(got[0]).sum() >= M.plan(q)["T"] and np.all(bits[np.isnan(got[0])] == 0x7FC00000)
    c.close()


# ---- 4: the second pass of the capped grid -----------------------------------------------------------------------------------------
def export_window(c, clip, channels, j0, j1):
    out, _ = c.clip_export(clip, "f32", channels, j0, j1 - j0, clamp=False)
    return [np.ascontiguousarray(out.reshape(-1, channels)[:, k]) for k in range(channels)]


def test_tiles_past_the_grid_cap():
    """2^16 + 3 tiles of 1024 outputs at the constant speed 1 / 24 (FAST, mono), so workgroups 0, 1 and 2 take a second
    tile and the source stays small.  Compared bit for bit: the first three tiles — the same workgroups' first pass —, the
    frames around tile 2^16's first, and everything from tile 2^16 - 2 to the end.  A call at another quality is made and
    freed first: the memory the result then gets held other frames, so a skipped tile shows."""
    G, g, q = 1 << 16, 10, M.FAST
    out = (G + 2) * 1024 + 301
    n = out // 24 + 40
    kn = M.constant_knots(out, g, 1, 24)
    t = W.varispeed_tiles(kn, g, n, out, q)
    assert len(t) == G + 3 and all(r[1] == 1024 for r in t[:-1]) and t[-1][1] == 301
    c = W.MixContext(4, block=128)
    seed, track, amp = 0x7A_5EED, 5, 0.75
    c.clip_synth(1, "f32", 1, RATE, n, seed, track, amp)
    plane = SP.SynthPlane(seed, track, 0, n, amp)
    c.clip_varispeed(1, 2, 0, n, out, kn, g, M.GOOD)              # fills the memory the result is about to get
    assert c.L.wbx_clip_free(c.h, 2) == 0
    c.clip_varispeed(1, 3, 0, n, out, kn, g, q)
    for j0, j1 in ((0, 3 * 1024), (G * 1024 - 2048, G * 1024 + 2048), ((G - 2) * 1024, out)):
        want = M.varispeed([plane], 0, n, out, kn, g, q, window=(j0, j1), tabs=tabs(q))
        got = export_window(c, 3, 1, j0, j1)
        bad = np.flatnonzero(got[0].view(np.uint32) != want[0].view(np.uint32))
        assert bad.size == 0 and got[0].size == j1 - j0 and np.any(want[0] != 0.0), (j0, bad[:8], bad.size)
    c.close()


# ---- 5: the pool, the refusals, the timer --------------------------------------------------------------------------------------------
def test_pool_replace_free_and_the_timer(ctx):
    out = 2051
    kn = M.constant_knots(out, 4, 5, 7)
    base = ctx.pool_stats()
    ctx.clip_varispeed(SRC[2], 120, 0, SRC_LEN, out, kn, 4, M.GOOD)
    with_one = ctx.pool_stats()
    ctx.clip_derive(SRC[2], 121, W.edit_desc(0, out))              # a plain copy of the same size takes the same
    assert (ctx.pool_stats()[2] - with_one[2]) == (with_one[2] - base[2])
    assert ctx.L.wbx_clip_free(ctx.h, 121) == 0
    for _ in range(3):                                             # a replaced dst takes the old extent
        ctx.clip_varispeed(SRC[2], 120, 3, SRC_LEN - 3, out, kn, 4, M.FAST)
        assert ctx.pool_stats() == with_one
    assert ctx.varispeed_ms() > 0.0
    assert ctx.L.wbx_clip_free(ctx.h, 120) == 0
    assert ctx.pool_stats() == base


def test_the_timer_needs_a_completed_call():
    c = W.MixContext(4, block=128)
    ms = C.c_double(5.0)
    assert c.L.wbx_varispeed_ms(c.h, C.byref(ms)) == -4 and ms.value == 5.0 and b"no varispeed call" in c.L.wbx_last_error(c.h)
    c.close()


def test_every_refusal_leaves_pool_dst_and_stats_untouched(ctx):
    L = W.lib()
    out, g = 64, 4
    good = M.constant_knots(out, g, 1, 1)
    ctx.clip_varispeed(SRC[2], DST, 0, SRC_LEN, out, good, g, M.FAST)
    kept = [p.view(np.uint32).tolist() for p in download(ctx, DST, 2, out)]
    ctx.clip_upload(5, "i16", RATE, [np.zeros(500, np.int16)] * 2)
    low, high, fast = good.copy(), good.copy(), good.copy()
    low[0] = -(M.MARGIN << 32) - 1
    high[-1] = ((SRC_LEN + M.MARGIN) << 32) + 1
    fast[3:] += 4100 * ONE
    TOP = (1 << 31) - 16
    base = dict(src=SRC[2], dst=DST, first=0, n=SRC_LEN, out=out, kn=good, nk=None, g=g, q=M.GOOD, gn=1, gd=1)
    cases = [(dict(n=0), -4, "no frames"), (dict(out=0), -4, "no frames"), (dict(n=TOP), -4, "2^31 - 16"), (dict(out=TOP), -4, "2^31 - 16"),
             (dict(g=3), -4, "knot_shift"), (dict(g=11), -4, "knot_shift"), (dict(kn=None), -4, "NULL"), (dict(nk=4), -4, "n_knots"),
             (dict(q=9), -4, "quality"), (dict(gn=0), -4, "guard of 0"), (dict(gd=0), -4, "guard of 0"), (dict(gn=2, gd=3), -4, "below 1"),
             (dict(gn=11), -3, "512 taps"), (dict(kn=low), -4, "a knot lies"), (dict(kn=high), -4, "a knot lies"),
             (dict(kn=fast), -3, "interval 2 moves too fast"), (dict(kn=fast), -3, "smaller knot_shift"),
             (dict(src=999), -4, "unknown source"), (dict(first=1), -4, "range ends past"), (dict(dst=SRC[2]), -4, "replace its source"),
             (dict(src=5, n=500), -3, "not F32"), (dict(dst=1 << 24), -4, "clip id"),
             # the order: sizes and curve before the clip, the range before the result's place before the storage, the id last
             (dict(n=0, g=3), -4, "no frames"), (dict(g=3, kn=None), -4, "knot_shift"), (dict(kn=None, nk=4), -4, "NULL"),
             (dict(nk=4, q=9), -4, "n_knots"), (dict(q=9, gn=0), -4, "quality"), (dict(gn=0, kn=low), -4, "guard of 0"),
             (dict(gn=11, kn=low), -3, "512 taps"), (dict(kn=low, src=999), -4, "a knot lies"), (dict(kn=fast, src=999), -3, "interval 2"),
             (dict(src=999, dst=999), -4, "unknown source"), (dict(src=5, n=501), -4, "range ends past"), (dict(src=5, dst=5, n=500), -4, "replace its source"),
             (dict(src=5, n=500, dst=1 << 24), -3, "not F32"), (dict(dst=1 << 24, first=1), -4, "range ends past")]
    before = ctx.pool_stats()
    for change, status, text in cases:
        a = dict(base, **change)
        st = _ffi.ClipStats()
        marks = bytes(st)
        kn = a["kn"]
        nk = a["nk"] if a["nk"] is not None else (0 if kn is None else len(kn))
        got = L.wbx_clip_varispeed(ctx.h, a["src"], a["dst"], a["first"], a["n"], a["out"], None if kn is None else kn.ctypes.data, nk,
                                   a["g"], a["q"], a["gn"], a["gd"], C.byref(st))
        assert got == status and text in L.wbx_last_error(ctx.h).decode(), (change, got, L.wbx_last_error(ctx.h))
        assert bytes(st) == marks and ctx.pool_stats() == before, change
    assert [p.view(np.uint32).tolist() for p in download(ctx, DST, 2, out)] == kept
    assert ctx.L.wbx_clip_free(ctx.h, 5) == 0


# ---- 6: layer 2 ------------------------------------------------------------------------------------------------------------------
def test_engine_entry_point_follows_the_sample_call_protocol():
    """the four points of tests/test_gpu_sample_calls.py for wbx_engine_varispeed_sample"""
    N = 4096
    eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
    eng.add_track("t")
    L = eng.L
    rng = np.random.default_rng(0x5A3)
    planes = [rng.uniform(-0.5, 0.5, N).astype(np.float32) for _ in range(2)]
    out = 3000
    kn = M.constant_knots(out, 5, 9, 8, start=50 * ONE + 77)

    def refused(call, status, message=None):
        with pytest.raises(W.WbxError) as err:
            call()
        assert err.value.status == status
        if message is not None:
            assert L.wbx_engine_last_error(eng.h).decode() == message

    # 1: an unknown id
    refused(lambda: eng.varispeed_sample(9999, out, kn, 5, first_frame=0, n_frames=N), -4, "varispeed_sample: unknown sample")
    # 2: a refusing check leaves no pin
    s = eng.add_sample("f32", RATE, planes)
    refused(lambda: eng.varispeed_sample(s, out, kn, 5, first_frame=1, n_frames=N), -4, "clip varispeed: the range ends past the clip")
    eng.delete_sample(s)
    rng16 = np.random.default_rng(0x116)
    s16 = eng.add_sample("i16", RATE, [rng16.integers(-20000, 20000, N).astype(np.int16) for _ in range(2)])
    refused(lambda: eng.varispeed_sample(s16, out, kn, 5, first_frame=0, n_frames=N), -3, "clip varispeed: the clip's storage format is not F32")
    eng.delete_sample(s16)
    # 3: a success is the pool's next id, registered with out_frames, the source's channels and rate
    s = eng.add_sample("f32", RATE, planes)
    n = N - 100
    new, st = eng.varispeed_sample(s, out, kn, 5, "good", 9, 8, first_frame=50, n_frames=n, stats=True)
    assert new == s + 1
    want = M.varispeed(planes, 50, n, out, kn, 5, M.GOOD, 9, 8)
    assert first_bad(download(eng.ctx, new, 2, out), want) is None
    check_stats(st, FX.measure(want), out, "engine")
    eng.measure_sample(new, 0, out, channels=2)
    refused(lambda: eng.measure_sample(new, 0, out + 1, channels=2), -4)
    assert eng._sample_rate.get(new, RATE) == RATE
    up = eng.resample_sample(new, 96000, "fast", 0, out)
    up_id = up[0] if isinstance(up, tuple) else up
    eng.measure_sample(up_id, 0, 2 * out, channels=2)              # registered at the source's rate: 48 kHz -> 96 kHz doubles it
    eng.delete_sample(s)
    # 4: a NULL new_sample
    s2 = eng.add_sample("f32", RATE, planes)
    assert L.wbx_engine_varispeed_sample(eng.h, s2, 0, N, out, kn.ctypes.data, len(kn), 5, 1, 9, 8, None, None) == -4
    assert L.wbx_engine_last_error(eng.h).decode() == "varispeed_sample: new_sample is NULL"
    eng.delete_sample(s2)
    eng.close()


def test_tape_stop_vibrato_and_drift_are_the_model_for_their_knots():
    N = 20000
    eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
    eng.add_track("t")
    t = np.arange(N, dtype=np.float64)
    planes = [(0.5 * np.sin(2 * np.pi * 440.0 * t / RATE + k) + 0.1 * np.sin(2 * np.pi * 9000.0 * t / RATE)).astype(np.float32) for k in range(2)]
    s = eng.add_sample("f32", RATE, planes)

    def same(new, info, q=M.GOOD):
        kn, g, out, guard = info["knots"], info["knot_shift"], info["out_frames"], info["guard"]
        assert M.check(kn, len(kn), g, N, out, q, *guard) == (0, "")
        want = M.varispeed(planes, 0, N, out, kn, g, q, *guard)
        got = download(eng.ctx, new, 2, out)
        assert first_bad(got, want) is None
        return got

    new, info = eng.tape_stop_sample(s, 12000, 6000)
    got = same(new, info)
    assert info["out_frames"] == 18000 and info["knots"][-1] <= 15001 * ONE and np.all(np.diff(info["knots"]) >= 0)
    tail = M.positions(info["knots"], info["knot_shift"], 17990, 18000)
    assert np.all(np.diff(tail) < ONE // 100)                      # the tape has all but stopped
    new, info = eng.vibrato_sample(s, 5.5, 50.0)
    same(new, info)
    speed = np.diff(info["knots"].astype(np.float64)) / (16 * ONE)
    assert info["out_frames"] == N and abs(speed.max() - 2 ** (50 / 1200)) < 1e-3 and abs(speed.min() - (2 - 2 ** (50 / 1200))) < 1e-3
    new, info = eng.drift_sample(s, 30.0)
    same(new, info)
    assert info["out_frames"] == round(N / 1.00003) and info["knots"][1] == (1024 * 100003 * ONE) // 100000
    new, info = eng.drift_sample(s, -2500.0, quality="best")
    same(new, info, M.BEST)
    assert info["out_frames"] == round(N / 0.9975)
    eng.close()


def test_pitch_curve_sample_is_warp_then_varispeed():
    N = 30000
    eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
    eng.add_track("t")
    t = np.arange(N, dtype=np.float64)
    planes = [(0.5 * np.sin(2 * np.pi * 220.0 * t / RATE + k)).astype(np.float32) for k in range(2)]
    s = eng.add_sample("f32", RATE, planes)
    before = set(eng._sample_shape)
    new, info = eng.pitch_curve_sample(s, [(0, 1.0), (10003, 2 ** (2 / 12)), (20000, 2 ** (-3 / 12))])
    assert info["out_frames"] == N and [m[0] for m in info["markers"]] == [10000, 20000]
    mid, _, _ = WM.warp_clip(planes, 0, N, info["mid_frames"], info["markers"])
    want = M.varispeed(mid, 0, info["mid_frames"], N, info["knots"], 4, M.GOOD, *info["guard"])
    assert first_bad(download(eng.ctx, new, 2, N), want) is None
    # every boundary keeps its frame: the curve passes through (boundary, marker) exactly
    for b, m in info["markers"]:
        assert M.position(info["knots"], 4, b) == m * ONE
    assert eng.L.wbx_engine_delete_sample(eng.h, new - 1) == -4      # the intermediate is gone
    assert set(eng._sample_shape) - before >= {new}
    eng.close()


def test_cpp_adapter_reads_a_take_along_a_curve(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_varispeed")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_varispeed.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "varispeed.bin")
    text = subprocess.check_output([exe, dump], timeout=120).decode()
    n, out, K = 5 * 512, 2000, 64
    assert "adapter varispeed ok %d knots %d" % (out, K) in text, text
    idx = np.arange(n, dtype=np.uint64)
    x = (((idx * 2654435761) & 0xFFFFFFFF) & 0xFFFF).astype(np.float32) / np.float32(65536.0) - np.float32(0.25)
    raw = open(dump, "rb").read()
    kn, got = np.frombuffer(raw[:8 * K], dtype=np.int64), np.frombuffer(raw[8 * K:], dtype=np.float32)
    assert kn[0] == 0 and kn[1] == 24 * ONE and kn[-1] - kn[-2] > 38 * ONE
    want = M.varispeed([x], 0, n, out, kn, 5, M.GOOD, 5, 4)
    assert got.size == out and first_bad([got], want) is None
    assert ("peak %.9g" % np.max(np.abs(want[0]))) in text, text


# ---- 7: beside the audio thread -------------------------------------------------------------------------------------------------
def test_varispeed_beside_the_audio_thread():
    """The shape of the saturate's test (test_gpu_saturate.py): a clip far behind the played range names the big source while
    the threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside one for
    the pin (-3, asked first) — one thread deletes without pause while the other reads along a curve until a delete has been
    refused for the pin.  The master is what it is without the calls, and the last result equals the model."""
    NB, FR, WAIT, CALLS = 300, 1 << 19, 60.0, 96
    spec = synth.make_session("vsthr", 2, n_blocks=NB, block=128, seed=0x7A7712)
    planes = source(2, FR, seed=41)

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
    out, g = 2 * n - 4001, 10
    kn = M.constant_knots(out, g, 1, 2, start=3 * ONE + 99)
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
                results["big"] = eng.varispeed_sample(big, out, kn, g, "best", 4, 1, first_frame=first, n_frames=n, channels=2, frames=FR)
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
    print("varispeed calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    j0 = out - 40000
    want = M.varispeed(planes, first, n, out, kn, g, M.BEST, 4, 1, window=(j0, out))
    got = [p[j0:] for p in download(eng.ctx, results["big"], 2, out)]
    assert first_bad(got, want) is None
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
